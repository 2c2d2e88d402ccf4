// Kernels that never touch a 16-bit operand, with their launchers: fp32 (and integer) in, fp32 out.  build.sh compiles this
// file ONCE, into namespace vl_once, and both builds of the 16-bit path (vl_f16 / vl_bf16: common.h), the fp32 parity mode and
// Swin-T call the one copy: the cross-entropy and DLR losses, the gradient scale, the classifier gradient, the FGSM / PGD step
// (K10), its random start (K11) and the zero fill, Auto-PGD (APGD-CE, APGD-T) and Square, flat Adam (K12), the save_images
// quantiser, the channel affine, the fp32 adapter fold and the dropout keep-mask.
// Every kernel moves 16 bytes per lane wherever the layout allows it.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "prof.h"
#include "once_kernels.h"

namespace vl_once {

namespace {

// F.cross_entropy(logits, labels), mean reduction; dlogits = (softmax - onehot)/B.
// one wave per image (4 per block) writes the per-image loss; a second tiny launch sums them in a
// fixed order (bitwise reproducible loss).
__global__ __launch_bounds__(256) void ce_loss_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                      int B, int C, float* __restrict__ dlogits, float* __restrict__ loss_img,
                                                      int* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int64_t yl = labels[b];
    if (yl < 0 || yl >= C) {               // refuse loudly: NaN loss for this image + the error word the next API call reports
        for (int c = lane; c < C; c += 64) dlogits[(int64_t)b * C + c] = __builtin_nanf("");
        if (lane == 0) { loss_img[b] = __builtin_nanf(""); if (err) *err = 1; }
        return;
    }
    const float* lr = logits + (int64_t)b * C;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, lr[c]);
    mx = wave_max(mx);
    float se = 0.f;
    for (int c = lane; c < C; c += 64) se += expf(lr[c] - mx);
    se = wave_sum(se);
    const int y = (int)yl;
    const float lse = mx + logf(se);
    for (int c = lane; c < C; c += 64)
        dlogits[(int64_t)b * C + c] = (expf(lr[c] - lse) - (c == y ? 1.f : 0.f)) / B;
    if (lane == 0) loss_img[b] = lse - lr[y];
}
__global__ __launch_bounds__(256) void ce_reduce_kernel(const float* __restrict__ loss_img, int B, float* __restrict__ loss_out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) s += loss_img[b];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *loss_out = (red[0] + red[1] + red[2] + red[3]) / B;
}

// per-image (one wave per image, four per block) or whole-batch (one block) max |dlogits| -> power-of-two scale that puts it
// in [2^9, 2^10)
__global__ __launch_bounds__(256) void grad_scale_kernel(const float* __restrict__ dlogits, int B, int C, int uniform,
                                                         float* __restrict__ gscale, float* __restrict__ inv_gscale) {
    __shared__ float red[4];
    auto scale_of = [](float mx) -> float {
        if (!(mx > 0.f) || !(mx < INFINITY)) return 1.f;          // all-zero or non-finite row: leave it alone
        int e;
        (void)frexpf(mx, &e);                                     // mx = f * 2^e, f in [0.5, 1)
        e = 10 - e;
        e = e < -60 ? -60 : (e > 60 ? 60 : e);
        return ldexpf(1.f, e);
    };
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (uniform) {
        float mx = 0.f;
        for (int i = threadIdx.x; i < B * C; i += 256) mx = fmaxf(mx, fabsf(dlogits[i]));
        mx = wave_max(mx);
        if (lane == 0) red[w] = mx;
        __syncthreads();
        const float sc = scale_of(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
        for (int b = threadIdx.x; b < B; b += 256) { gscale[b] = sc; inv_gscale[b] = 1.f / sc; }
        return;
    }
    // (a single block walking 64 images per wave was 38 us of dependent load latency per PGD iteration at batch 256)
    for (int b = blockIdx.x * 4 + w; b < B; b += 4 * gridDim.x) {
        float mx = 0.f;
        for (int c = lane; c < C; c += 64) mx = fmaxf(mx, fabsf(dlogits[(int64_t)b * C + c]));
        mx = wave_max(mx);
        if (lane == 0) { const float sc = scale_of(mx); gscale[b] = sc; inv_gscale[b] = 1.f / sc; }
    }
}

// classifier gradient (train): dW[c][d] = sum_b dlogits[b][c] * xf[b][d]; db[c] = sum_b dlogits[b][c]
__global__ void classifier_grad_kernel(const float* __restrict__ dlogits, const float* __restrict__ xf, int B, int D,
                                       int C, float* __restrict__ dW, float* __restrict__ db) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < C * D) {
        const int c = i / D, d = i - c * D;
        float a = 0.f;
        for (int b = 0; b < B; ++b) a += dlogits[(int64_t)b * C + c] * xf[(int64_t)b * D + d];
        dW[i] = a;
    }
    if (i < C) {
        float a = 0.f;
        for (int b = 0; b < B; ++b) a += dlogits[(int64_t)b * C + i];
        db[i] = a;
    }
}

// ---------------------------------------------------------------------------------
// K10: fused input-grad -> sign -> eps-project -> clamp.  16 B/elem algorithmic traffic
// (reads g, adv, x0; writes adv).  whitebox_attacks.py:32-36 (FGSM) / torchattacks PGD step.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ float sgn(float g) { return (g > 0.f) ? 1.f : ((g < 0.f) ? -1.f : 0.f); }

// Access shape (round 5, tools/k10_sweep.hip on MI355X, 616.6 MB per launch): the three input streams are read with
// NON-TEMPORAL 16-byte loads, two vectors per thread in flight, plain stores: 92 us = 6.7 TB/s = 0.84 of the 8 TB/s peak
// (plain loads, rounds 1-4: 112-119 us = 0.65-0.69; a float4 copy reaches 5.5 TB/s on the same box; non-temporal STORES lose
// the gain again: 106 us).  Every byte is used once, so nothing is lost by not keeping the lines.
__global__ __launch_bounds__(256) void pgd_step_kernel(float* __restrict__ adv, const float* __restrict__ x0,
                                                       const float* __restrict__ grad, float eps, float alpha,
                                                       float lo, float hi, int64_t n4, int64_t n, int* __restrict__ err) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += 2 * stride) {
        const int64_t j = i + stride;
        const bool two = j < n4;
        const f32x4 a0 = __builtin_nontemporal_load((const f32x4*)adv + i);
        const f32x4 x0v = __builtin_nontemporal_load((const f32x4*)x0 + i);
        const f32x4 g0 = __builtin_nontemporal_load((const f32x4*)grad + i);
        f32x4 a1 = a0, x1v = x0v, g1 = g0;
        if (two) {
            a1 = __builtin_nontemporal_load((const f32x4*)adv + j);
            x1v = __builtin_nontemporal_load((const f32x4*)x0 + j);
            g1 = __builtin_nontemporal_load((const f32x4*)grad + j);
        }
        bool bad = false;
        f32x4 o0, o1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bad |= !(fabsf(g0[k]) < INFINITY) | !(fabsf(g1[k]) < INFINITY);
            const float t0 = a0[k] + alpha * sgn(g0[k]);
            const float d0 = fminf(fmaxf(t0 - x0v[k], -eps), eps);
            o0[k] = fminf(fmaxf(x0v[k] + d0, lo), hi);
            const float t1 = a1[k] + alpha * sgn(g1[k]);
            const float d1 = fminf(fmaxf(t1 - x1v[k], -eps), eps);
            o1[k] = fminf(fmaxf(x1v[k] + d1, lo), hi);
        }
        if (err && bad) *err = 2;
        *((f32x4*)adv + i) = o0;
        if (two) *((f32x4*)adv + j) = o1;
    }
    // tail (n not a multiple of 4)
    const int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) {
        const float t = adv[i] + alpha * sgn(grad[i]);
        const float d = fminf(fmaxf(t - x0[i], -eps), eps);
        adv[i] = fminf(fmaxf(x0[i] + d, lo), hi);
    }
}

// Zero fill (bytes a multiple of 16, 16-byte aligned).  Used INSIDE captured sequences instead of hipMemsetAsync: a memset
// node captured before the runtime's own fill kernel had ever run did not take effect on graph replays (ROCm 7.2;
// tools/cold_capture_diag.py), a kernel node of the library's own code object does.
__global__ __launch_bounds__(256) void zero_kernel(f32x4* __restrict__ p, int64_t n16) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n16; i += stride) p[i] = z;
}

// K11: counter-based uniform noise (splitmix64 finaliser on (seed, index)); not torch's stream
// (random_start=True, whitebox_attacks.py:113, needs a seeded deterministic start, not that stream).
// (mix64 lives in common.h: the LoRA dropout mask uses the same generator)
__global__ void pgd_init_kernel(float* __restrict__ adv, const float* __restrict__ x0, float eps, float lo, float hi,
                                uint64_t seed, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t r = mix64(seed * 0xD1342543DE82EF95ull + (uint64_t)i);
        const float u = (float)(r >> 40) * (1.0f / 16777216.0f);       // [0,1)
        const float v = x0[i] + (2.f * u - 1.f) * eps;
        adv[i] = fminf(fmaxf(v, lo), hi);
    }
}

// ---------------------------------------------------------------------------------
// Auto-PGD (APGD-CE, L-inf; Croce & Hein 2020).  The algorithm is the restatement in DESIGN.md section 3.9 -- written from
// memory of the autoattack package's autopgd_base.py, which is not installed here: parity with the package is UNPINNED.
// One captured iteration (forward, CE, backward, apgd_track_kernel, apgd_step_kernel) serves every iteration index: what
// differs between iterations (momentum, checkpoint, first / last) is read from a schedule table at a device-side counter.
// The counter is two words: the track kernel reads ctr[0] and writes ctr[1] = ctr[0] + 1, the step kernel reads ctr[1] and
// writes ctr[0] = ctr[1] -- no kernel reads a word that one of its own blocks writes.
// ---------------------------------------------------------------------------------
// Schedule table entry j (replay j evaluates the point of iteration j - 1 and makes the point of iteration j) and the counter.
__global__ void apgd_sched_kernel(ApgdSched* __restrict__ sched, int32_t* __restrict__ ctr, int N, int k0, int kmin, int dec) {
    if (blockIdx.x || threadIdx.x) return;
    int k = k0, cnt = 0;
    sched[0] = {1.f, 0, APGD_FIRST | (N == 0 ? APGD_LAST : 0), 0};
    for (int i = 0; i < N; ++i) {               // iteration i is evaluated by replay i + 1
        ApgdSched e = {0.75f, 0, i + 1 == N ? APGD_LAST : 0, 0};     // a of iteration i + 1 (iteration 0 alone has a = 1)
        if (++cnt == k) { e.k = k; k = k - dec > kmin ? k - dec : kmin; cnt = 0; }
        sched[i + 1] = e;
    }
    ctr[0] = 0; ctr[1] = 0; ctr[2] = 0; ctr[3] = 0;
}

// start = x0 + eps * t / max|t|, t ~ U(-1, 1) from the counter-based generator, the maximum taken per image; one block per image
__global__ __launch_bounds__(256) void apgd_rand_init_kernel(float* __restrict__ x_adv, const float* __restrict__ x0, float eps,
                                                              uint64_t seed, int64_t n) {
    __shared__ float red[4];
    const int64_t base = (int64_t)blockIdx.x * n;
    auto draw = [&](int64_t i) -> float {
        const uint64_t r = mix64(seed * 0xD1342543DE82EF95ull + (uint64_t)(base + i));
        return 2.f * ((float)(r >> 40) * (1.0f / 16777216.0f)) - 1.f;
    };
    float mx = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) mx = fmaxf(mx, fabsf(draw(i)));
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    mx = mx > 0.f ? mx : 1.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const float v = x0[base + i] + (eps * draw(i)) / mx;
        x_adv[base + i] = fminf(fmaxf(v, 0.f), 1.f);
    }
}

// x_adv = clamp(start, 0, 1) for a start point the caller gives (x0 itself or x_init)
__global__ void apgd_start_kernel(float* __restrict__ x_adv, const float* __restrict__ src, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) x_adv[i] = fminf(fmaxf(src[i], 0.f), 1.f);
}

// Steps 2-4 of one iteration for one image per wave (four per block): prediction from the logits row, best-loss and robust
// bookkeeping, the checkpoint test, the new step size; writes the flag word the step kernel acts on and the trace rows.
__global__ __launch_bounds__(256) void apgd_track_kernel(ApgdState st, const float* __restrict__ loss_img,
                                                         const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                         int B, int C, int N, float eps, float rho) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int j = st.ctr[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) st.ctr[1] = j + 1;
    if (b >= B || (unsigned)j > (unsigned)N) return;     // a replay past the table does nothing
    const ApgdSched e = st.sched[j];
    // pred = (argmax == y), the first maximum as torch.argmax
    const float* lr = logits + (int64_t)b * C;
    float mx = -INFINITY;
    int am = 0x7fffffff;
    for (int c = lane; c < C; c += 64) { const float v = lr[c]; if (v > mx) { mx = v; am = c; } }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(mx, o, 64);
        const int oa = __shfl_xor(am, o, 64);
        if (ov > mx || (ov == mx && oa < am)) { mx = ov; am = oa; }
    }
    const int pred = ((int64_t)am == labels[b]) ? 1 : 0;
    const float loss = loss_img[b];
    float step, lb, lbl;
    int red_last, rob;
    uint32_t fl = 0;
    if (e.flags & APGD_FIRST) {        // the start point: x_best = x_best_adv = x_adv, grad_best = grad
        step = 2.f * eps; lb = loss; lbl = loss; red_last = 1; rob = pred;
        fl = APGD_IMPROVED | APGD_FOOLED;
    } else {
        step = st.step[b]; lb = st.loss_best[b]; lbl = st.loss_best_last[b]; red_last = st.reduced_last[b];
        rob = st.robust[b] & pred;
        if (!pred) fl |= APGD_FOOLED;
        if (loss > lb) { lb = loss; fl |= APGD_IMPROVED; }
        if (e.k > 0) {                 // checkpoint: loss_steps[i] is trace row i + 1, row "-1" reads 0
            const int i = j - 1;
            int t = 0;
            for (int c = lane; c < e.k; c += 64) {
                const int hi = i - c, lo = hi - 1;
                const float vh = hi == i ? loss : (hi < 0 ? 0.f : st.tr_loss[(int64_t)(hi + 1) * B + b]);
                const float vl = lo < 0 ? 0.f : st.tr_loss[(int64_t)(lo + 1) * B + b];
                t += vh > vl ? 1 : 0;
            }
            t = (int)wave_sum((float)t);
            const bool osc = (float)t <= (float)e.k * rho;
            const bool noimp = !red_last && lbl >= lb;
            const bool red = osc || noimp;
            red_last = red ? 1 : 0;
            lbl = lb;
            if (red) { step = step * 0.5f; fl |= APGD_RESTART; }
        }
    }
    if (lane == 0) {
        st.step[b] = step; st.loss_best[b] = lb; st.loss_best_last[b] = lbl; st.reduced_last[b] = red_last;
        st.robust[b] = rob; st.flags[b] = fl;
        st.tr_loss[(int64_t)j * B + b] = loss;
        st.tr_pred[(int64_t)j * B + b] = pred;
        if (j < N) st.tr_step[(int64_t)j * B + b] = step;      // the step size iteration j's update uses
    }
}

// P(v) = clamp(min(max(v, x0 - eps), x0 + eps), 0, 1); z = P(xa + step sign(g)); new = P((xa + (z - xa) a) + g2 (1 - a)),
// every operation rounded on its own (no FMA contraction: the reference restatement is bit-exact)
__device__ __forceinline__ float apgd_update(float xa, float xo, float x0, float g, float step, float eps, float a, float oma) {
#pragma clang fp contract(off)
    const float lo = x0 - eps, hi = x0 + eps;
    const float g2 = xa - xo;
    const float v = xa + step * sgn(g);
    const float z = fminf(fmaxf(fminf(fmaxf(v, lo), hi), 0.f), 1.f);
    const float d = (z - xa) * a;
    const float m = g2 * oma;
    const float w = (xa + d) + m;
    return fminf(fmaxf(fminf(fmaxf(w, lo), hi), 0.f), 1.f);
}

// The elementwise pass of one iteration: blockIdx.y = image, so the flag branches are uniform over the block.  In ONE read of
// x_adv, x_old, x0 and grad: the copies the track kernel asked for (improved: x_best, grad_best <- x_adv, grad; fooled:
// x_best_adv <- x_adv; restart: x_adv, grad <- x_best, grad_best -- after the improved copy, so both together leave x_adv as it
// is), then step 1 of the NEXT iteration (x_old <- x_adv, x_adv <- new point) unless this is the last evaluation.  24 B per
// element (four 16-byte non-temporal loads, two stores; pgd_step_kernel's access shape) plus the copies where a flag is set.
// sched != nullptr: a / last come from the table entry at ctr[1] - 1; nullptr: from the arguments (vl_apgd_step).
__global__ __launch_bounds__(256) void apgd_step_kernel(float* __restrict__ x_adv, float* __restrict__ x_old,
                                                        float* __restrict__ x_best, float* __restrict__ x_best_adv,
                                                        float* __restrict__ grad_best, const float* __restrict__ x0,
                                                        const float* __restrict__ grad, const uint32_t* __restrict__ flags,
                                                        const float* __restrict__ step, int64_t n4, float eps,
                                                        const ApgdSched* __restrict__ sched, int32_t* __restrict__ ctr, int N,
                                                        float a, int last, int* __restrict__ err) {
#pragma clang fp contract(off)
    if (sched) {
        const int j = ctr[1] - 1;
        if ((unsigned)j > (unsigned)N) return;
        a = sched[j].a;
        last = sched[j].flags & APGD_LAST;
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) ctr[0] = j + 1;
    }
    const int b = blockIdx.y;
    const uint32_t fl = flags[b];
    const float st = step[b];
    const float oma = 1.f - a;
    const bool improved = fl & APGD_IMPROVED, fooled = fl & APGD_FOOLED, restart = (fl & APGD_RESTART) && !improved;
    if (last && !improved && !fooled) return;        // nothing to copy, no further point to make
    const int64_t base = (int64_t)b * n4;
    f32x4* const pa = (f32x4*)x_adv + base;
    f32x4* const po = (f32x4*)x_old + base;
    f32x4* const pb = (f32x4*)x_best + base;
    f32x4* const pf = (f32x4*)x_best_adv + base;
    f32x4* const pg = (f32x4*)grad_best + base;
    const f32x4* const p0 = (const f32x4*)x0 + base;
    const f32x4* const pgr = (const f32x4*)grad + base;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += 2 * stride) {
        const int64_t k = i + stride;
        const bool two = k < n4;
        f32x4 a0 = __builtin_nontemporal_load(pa + i);
        const f32x4 o0 = __builtin_nontemporal_load(po + i);
        const f32x4 x0v = __builtin_nontemporal_load(p0 + i);
        f32x4 g0 = __builtin_nontemporal_load(pgr + i);
        f32x4 a1 = a0, o1 = o0, x1v = x0v, g1 = g0;
        if (two) {
            a1 = __builtin_nontemporal_load(pa + k);
            o1 = __builtin_nontemporal_load(po + k);
            x1v = __builtin_nontemporal_load(p0 + k);
            g1 = __builtin_nontemporal_load(pgr + k);
        }
        bool bad = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) bad |= !(fabsf(g0[q]) < INFINITY) | !(fabsf(g1[q]) < INFINITY);
        if (err && bad) *err = 2;
        if (improved) { pb[i] = a0; pg[i] = g0; if (two) { pb[k] = a1; pg[k] = g1; } }
        if (fooled) { pf[i] = a0; if (two) pf[k] = a1; }
        if (last) continue;
        if (restart) { a0 = pb[i]; g0 = pg[i]; if (two) { a1 = pb[k]; g1 = pg[k]; } }
        f32x4 n0, n1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            n0[q] = apgd_update(a0[q], o0[q], x0v[q], g0[q], st, eps, a, oma);
            n1[q] = apgd_update(a1[q], o1[q], x1v[q], g1[q], st, eps, a, oma);
        }
        po[i] = a0; pa[i] = n0;
        if (two) { po[k] = a1; pa[k] = n1; }
    }
}

// ---------------------------------------------------------------------------------
// APGD-T (targeted Auto-PGD on the DLR loss; DESIGN.md section 3.11 -- a restatement of the autoattack package's
// APGDAttack_targeted from memory: parity with the package is UNPINNED).  The iteration is APGD's with another loss kernel;
// apgd_track_kernel and apgd_step_kernel are reused unchanged ("fooled" stays argmax != label).
// ---------------------------------------------------------------------------------
// The wave's best (value, index) in the order "value descending, index ascending"; NO_IDX marks "no candidate".  Every lane
// returns lane 0's result, so the lanes agree even on a row that holds NaN.
constexpr int NO_IDX = 0x7fffffff;
__device__ __forceinline__ bool ranks_before(float v, int c, float bv, int bc) {
    return c != NO_IDX && (bc == NO_IDX || v > bv || (v == bv && c < bc));
}
__device__ __forceinline__ void wave_best(float& v, int& c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oc = __shfl_xor(c, o, 64);
        if (ranks_before(ov, oc, v, c)) { v = ov; c = oc; }
    }
    v = __shfl(v, 0, 64);
    c = __shfl(c, 0, 64);
}

// DLR-targeted loss, one wave per image (four per block), any C >= 4: pi1 .. pi4 by four wave arg-max passes, each over the
// classes that rank strictly after the previous pick.  N = z_y - z_t, D = (z_pi1 - (z_pi3 + z_pi4) / 2) + 1e-12, q = N / D,
// loss = -q, and the row written is  D * dloss/dz = -[(d_cy - d_ct) - q (d_c,pi1 - d_c,pi3 / 2 - d_c,pi4 / 2)]:
// the positive per-image factor D is DELIBERATE -- only the sign of the input gradient is used and the backward rescales each
// image anyway (grad_scale_kernel); without it a near-tie among the top four classes puts 1 / D^2, about 1e24, into the row.
// Every operation is rounded on its own, in this order (no FMA contraction: the float32 restatement in tests/apgdt_ref.py is
// bit-exact).  A label outside [0, C): NaN row, NaN loss, *err = 1 (as ce_loss_kernel); a target outside [0, C) or equal to the
// label: the same with *err = 6.
__global__ __launch_bounds__(256) void dlr_targeted_loss_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                                const int32_t* __restrict__ targets, int B, int C,
                                                                float* __restrict__ dlogits, float* __restrict__ loss_img,
                                                                int* __restrict__ err) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int64_t yl = labels[b];
    const int t = targets[b];
    const bool bad_label = yl < 0 || yl >= C, bad_target = t < 0 || t >= C || (int64_t)t == yl;
    if (bad_label || bad_target) {
        for (int c = lane; c < C; c += 64) dlogits[(int64_t)b * C + c] = __builtin_nanf("");
        if (lane == 0) { loss_img[b] = __builtin_nanf(""); if (err) *err = bad_label ? 1 : 6; }
        return;
    }
    const int y = (int)yl;
    const float* lr = logits + (int64_t)b * C;
    float pv[4];
    int pc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float bv = 0.f;
        int bc = NO_IDX;
        for (int c = lane; c < C; c += 64) {
            const float v = lr[c];
            const bool after = k == 0 || ranks_before(pv[k ? k - 1 : 0], pc[k ? k - 1 : 0], v, c);      // strictly after the previous pick
            if (after && ranks_before(v, c, bv, bc)) { bv = v; bc = c; }
        }
        wave_best(bv, bc);
        if (bc == NO_IDX) { bv = k ? pv[k ? k - 1 : 0] : 0.f; bc = k ? pc[k ? k - 1 : 0] : 0; }      // only on a row that holds NaN: stay inside the row
        pv[k] = bv; pc[k] = bc;
    }
    const float n = lr[y] - lr[t];
    const float h = (pv[2] + pv[3]) * 0.5f;
    const float d = (pv[0] - h) + 1e-12f;
    const float q = n / d;
    for (int c = lane; c < C; c += 64) {
        const float a = (c == y ? 1.f : 0.f) - (c == t ? 1.f : 0.f);
        const float w = ((c == pc[0] ? 1.f : 0.f) - (c == pc[2] ? 0.5f : 0.f)) - (c == pc[3] ? 0.5f : 0.f);
        dlogits[(int64_t)b * C + c] = -(a - q * w);
    }
    if (lane == 0) loss_img[b] = -q;
}

// Target classes of APGD-T, one wave per image (four per block): clean_correct = (first maximum == label), then n_target times
// the arg-max over the classes != label that rank strictly after the previous pick (value descending, index ascending).
// n_target <= C - 1, so every pick exists unless the row holds NaN (then -1, which the loss kernel refuses).
__global__ __launch_bounds__(256) void apgd_targets_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                           int B, int C, int n_target, int32_t* __restrict__ targets,
                                                           int32_t* __restrict__ clean_correct) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int64_t yl = labels[b];
    const float* lr = logits + (int64_t)b * C;
    float pv = 0.f;
    int pc = NO_IDX;
    for (int c = lane; c < C; c += 64) { const float v = lr[c]; if (ranks_before(v, c, pv, pc)) { pv = v; pc = c; } }
    wave_best(pv, pc);
    if (lane == 0) clean_correct[b] = ((int64_t)pc == yl) ? 1 : 0;
    pc = NO_IDX;
    for (int k = 0; k < n_target; ++k) {
        float bv = 0.f;
        int bc = NO_IDX;
        for (int c = lane; c < C; c += 64) {
            const float v = lr[c];
            const bool after = pc == NO_IDX || ranks_before(pv, pc, v, c);
            if ((int64_t)c != yl && after && ranks_before(v, c, bv, bc)) { bv = v; bc = c; }
        }
        wave_best(bv, bc);
        if (lane == 0) targets[(int64_t)k * B + b] = bc == NO_IDX ? -1 : bc;
        if (bc == NO_IDX) { for (int j = k + 1; j < n_target; ++j) if (lane == 0) targets[(int64_t)j * B + b] = -1; return; }
        pv = bv; pc = bc;
    }
}

// The fold over runs: blockIdx.y = image, so the branch is uniform over the block.  An image that was still robust and that this
// run fooled takes the run's misclassified point (16-byte copies) and records the run; still_out = still_in & run_robust.  still_in
// and still_out are two arrays, so no block reads a word that another block writes.
__global__ __launch_bounds__(256) void apgdt_fold_kernel(float* __restrict__ x_out, const float* __restrict__ x_best_adv,
                                                         const int32_t* __restrict__ still_in, int32_t* __restrict__ still_out,
                                                         const int32_t* __restrict__ run_robust, int32_t* __restrict__ fooled_by,
                                                         int run, int64_t n4) {
    const int b = blockIdx.y;
    const bool still = still_in[b] != 0, rob = run_robust[b] != 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        still_out[b] = (still && rob) ? 1 : 0;
        if (still && !rob) fooled_by[b] = run;
    }
    if (!still || rob) return;
    const int64_t base = (int64_t)b * n4;
    const f32x4* const src = (const f32x4*)x_best_adv + base;
    f32x4* const dst = (f32x4*)x_out + base;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += stride) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------
// Square attack (Andriushchenko et al. 2020; L-inf, untargeted margin loss, rescaled schedule).  The algorithm is the restatement
// in DESIGN.md section 3.10 -- written from memory of the autoattack package's square.py and the paper, neither installed here:
// parity with the package is UNPINNED.  Two deliberate deviations: the window and its signs are drawn PER IMAGE (an image's
// random stream depends on its global index alone, not on its neighbours or the batch cut), and the window is written as
// clamp(x0 +- eps, 0, 1) directly.  One captured iteration (eval forward of x_cur, square_track_kernel, square_step_kernel)
// serves every replay; the replay index is the two-word counter of the APGD kernels above (the track kernel reads ctr[0] and
// writes ctr[1], the step kernel reads ctr[1] and writes ctr[0]).  Seed and image offset are read from the scratch, not passed
// as arguments, so one captured iteration serves every seed.
//   r(g, j, k) = mix64(key ^ (g << 32) ^ (j << 2) ^ k),  g = the image's global index, k = 0 row, 1 column, 2 signs, 3 stripes
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t square_draw(uint64_t key, uint64_t g, uint32_t j, uint32_t k) {
    return mix64(key ^ (g << 32) ^ ((uint64_t)j << 2) ^ (uint64_t)k);
}

// side[j] of proposal j = 1 .. N from the (first proposal, side) pairs; the counter; key and image offset
__global__ __launch_bounds__(256) void square_sched_kernel(SquareState st, SquareSched sc, int N, uint64_t seed, uint64_t offset) {
    for (int j = threadIdx.x; j <= N; j += 256) {
        int k = 0;
#pragma unroll
        for (int i = 1; i < 10; ++i) k = j >= sc.from[i] ? i : k;
        st.side[j] = sc.side[k];
    }
    if (threadIdx.x == 0) {
        st.ctr[0] = 0; st.ctr[1] = 0; st.ctr[2] = 0; st.ctr[3] = 0;
        st.par->key = seed * 0xD1342543DE82EF95ull;
        st.par->offset = offset;
    }
}

// the start point: vertical stripes, one sign per (image, channel, column), written into x_cur and x_best; blockIdx.y = image
__global__ __launch_bounds__(256) void square_init_kernel(float* __restrict__ x_cur, float* __restrict__ x_best,
                                                          const float* __restrict__ x0, const SquareParams* __restrict__ par,
                                                          int S, float eps) {
    const uint64_t key = par->key, g = par->offset + blockIdx.y;
    const int n = 3 * S * S;
    const int64_t base = (int64_t)blockIdx.y * n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int c = i / (S * S), col = i % S;
        const bool up = (square_draw(key, g, (uint32_t)(c * S + col), 3) >> 40) & 1;
        const float x = x0[base + i];
        const float v = fminf(fmaxf(up ? x + eps : x - eps, 0.f), 1.f);
        x_cur[base + i] = v;
        x_best[base + i] = v;
    }
}

// One replay's bookkeeping for one image per wave (four per block): the margin z_y - max_{j != y} z_j from the logits row,
// accept / reject of the pending proposal, margin_min and the query count, then the next proposal unless the image is frozen
// (margin_min <= 0) or this is the last replay.  A margin that is not finite is never accepted and raises the error word.
__global__ __launch_bounds__(256) void square_track_kernel(SquareState st, const float* __restrict__ logits,
                                                           const int64_t* __restrict__ labels, int B, int C, int S, int N,
                                                           int* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int j = st.ctr[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) st.ctr[1] = j + 1;
    if (b >= B || (unsigned)j > (unsigned)N) return;     // a replay past the schedule does nothing
    const int64_t y = labels[b];
    const bool ybad = y < 0 || y >= C;
    const float* lr = logits + (int64_t)b * C;
    float mx = -INFINITY;
    int bad = 0;
    for (int c = lane; c < C; c += 64) {
        if (c == y) continue;
        const float v = lr[c];
        bad |= v != v;
        mx = fmaxf(mx, v);
    }
    mx = wave_max(mx);
    bad = __any(bad);
    if (lane) return;
    const float m = (ybad || bad) ? NAN : lr[y] - mx;
    const bool finite = fabsf(m) < INFINITY;
    if (!finite && err) *err = ybad ? 1 : 5;
    float mm;
    int q;
    uint32_t fl = 0;
    int32_t* const wp = st.win_prev + 4 * b;
    int32_t* const wn = st.win_next + 4 * b;
    if (j == 0) {                                // the stripes
        mm = finite ? m : INFINITY;
        q = 1;
    } else {
        mm = st.margin_min[b];
        q = st.queries[b];
        if (st.flags[b] & SQ_NEXT) {             // proposal j was made for this image: this replay evaluated it
            ++q;
            fl |= SQ_PREV;
            wp[0] = wn[0]; wp[1] = wn[1]; wp[2] = wn[2]; wp[3] = wn[3];
            if (finite && m < mm) {
                mm = m;
                fl |= SQ_ACCEPT;
                st.tr_win[((int64_t)(j - 1) * B + b) * 4 + 3] |= 16;
            }
        }
    }
    if (j < N) {
        int32_t* const tw = st.tr_win + ((int64_t)j * B + b) * 4;
        if (mm > 0.f) {                          // still active: proposal j + 1
            const uint64_t key = st.par->key, g = st.par->offset + (uint64_t)b;
            const int s = st.side[j + 1];
            const uint64_t span = (uint64_t)(S - s + 1);
            const int h = (int)(((square_draw(key, g, (uint32_t)(j + 1), 0) >> 32) * span) >> 32);
            const int w = (int)(((square_draw(key, g, (uint32_t)(j + 1), 1) >> 32) * span) >> 32);
            const int sg = (int)((square_draw(key, g, (uint32_t)(j + 1), 2) >> 40) & 7);
            wn[0] = h; wn[1] = w; wn[2] = s; wn[3] = sg;
            tw[0] = h; tw[1] = w; tw[2] = s; tw[3] = sg | 8;
            fl |= SQ_NEXT;
        } else {
            tw[0] = 0; tw[1] = 0; tw[2] = 0; tw[3] = 0;
        }
    }
    st.margin_min[b] = mm; st.queries[b] = q; st.robust[b] = mm > 0.f ? 1 : 0; st.flags[b] = fl;
    st.tr_margin[(int64_t)j * B + b] = m;
}

// The pixel pass of one replay: blockIdx.y = image, so the flag branches are uniform over the block.  Only the union of the
// previous and the next window is touched (3 (s_prev^2 + s_next^2) work items, never the whole image).  Item t < 3 s_prev^2 is a
// pixel of the previous window: its thread resolves it (accept: x_best <- x_cur; reject: x_cur <- x_best) and, where the pixel
// also lies in the next window, writes the new value afterwards.  The remaining items are the pixels of the next window; those
// inside the previous window are skipped -- their owner is the thread above -- so every pixel of the union has exactly one owner
// and overlapping windows cannot race.  Windows start at any column and have any width: plain dword accesses.
// A window that does not fit the image is ignored (vl_square_step takes windows from the caller).
__global__ __launch_bounds__(256) void square_step_kernel(float* __restrict__ x_cur, float* __restrict__ x_best,
                                                          const float* __restrict__ x0, const uint32_t* __restrict__ flags,
                                                          const int32_t* __restrict__ win_prev, const int32_t* __restrict__ win_next,
                                                          int S, float eps, int32_t* __restrict__ ctr, int N) {
    if (ctr) {
        const int j = ctr[1] - 1;
        if ((unsigned)j > (unsigned)N) return;
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) ctr[0] = j + 1;
    }
    const int b = blockIdx.y;
    const uint32_t fl = flags[b];
    const bool acc = fl & SQ_ACCEPT;
    int ph = win_prev[4 * b], pw = win_prev[4 * b + 1], ps = win_prev[4 * b + 2];
    int nh = win_next[4 * b], nw = win_next[4 * b + 1], ns = win_next[4 * b + 2];
    const int nsg = win_next[4 * b + 3];
    if (!(fl & SQ_PREV) || ps <= 0 || ps > S || ph < 0 || pw < 0 || ph > S - ps || pw > S - ps) ps = 0;
    if (!(fl & SQ_NEXT) || ns <= 0 || ns > S || nh < 0 || nw < 0 || nh > S - ns || nw > S - ns) ns = 0;
    const int np = 3 * ps * ps, total = np + 3 * ns * ns;
    const int64_t base = (int64_t)b * 3 * S * S;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
        const bool first = t < np;
        const int u = first ? t : t - np, s = first ? ps : ns;
        const int c = u / (s * s), rem = u - c * s * s, r = rem / s;
        const int row = (first ? ph : nh) + r, col = (first ? pw : nw) + (rem - r * s);
        const int64_t i = base + ((int64_t)c * S + row) * S + col;
        if (first) {
            if (acc) x_best[i] = x_cur[i];
            else x_cur[i] = x_best[i];
            if (!(row >= nh && row < nh + ns && col >= nw && col < nw + ns)) continue;     // ns == 0: never inside
        } else if (row >= ph && row < ph + ps && col >= pw && col < pw + ps) {
            continue;
        }
        const float x = x0[i];
        x_cur[i] = fminf(fmaxf(((nsg >> c) & 1) ? x + eps : x - eps, 0.f), 1.f);
    }
}

// K12: torch.optim.Adam single flat update (train_loras.py:284,315)
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, float lr, float b1, float b2, float eps, float bc1,
                            float sqrt_bc2, int64_t n, int* __restrict__ err) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    if (!(fabsf(gi) < INFINITY)) {           // non-finite gradient: leave the parameter and its moments alone, report it
        if (err) *err = 3;
        return;
    }
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / sqrt_bc2 + eps;
    p[i] -= (lr / bc1) * (mi / denom);
}

// save_images (Utils.py:108-112): clamp(0,1) -> *255 -> uint8 truncation, CHW -> HWC
__global__ void quantize_kernel(const float* __restrict__ img, uint8_t* __restrict__ out, int B, int Cn, int H, int W) {
    const int64_t n = (int64_t)B * Cn * H * W;
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    // i indexes the OUTPUT (b, y, x, c)
    const int c = (int)(i % Cn);
    int64_t r = i / Cn;
    const int xx = (int)(r % W); r /= W;
    const int yy = (int)(r % H);
    const int b = (int)(r / H);
    float v = img[(((int64_t)b * Cn + c) * H + yy) * W + xx];
    v = fminf(fmaxf(v, 0.f), 1.f);
    out[i] = (uint8_t)(v * 255.f);
}

__global__ void channel_affine_kernel(float* __restrict__ dst, const float* __restrict__ src, float s0, float s1,
                                      float s2, float t0, float t1, float t2, int64_t hw, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
        const int c = (int)((i / hw) % 3);
        const float sc = c == 0 ? s0 : (c == 1 ? s1 : s2), sh = c == 0 ? t0 : (c == 1 ? t1 : t2);
        dst[i] = src[i] * sc + sh;
    }
}

// fp32 form of merge_lora_kernel's fold (elementwise.hip): W + s B A (adapter composition: the merged weight becomes the next base)
__global__ void merge_f32_kernel(const float* __restrict__ W, const float* __restrict__ A, const float* __restrict__ Bm,
                                 int out, int in, int r, float s, float* __restrict__ dst) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= (int64_t)out * in) return;
    const int o = (int)(i / in), k = (int)(i - (int64_t)o * in);
    float a = 0.f;
    for (int j = 0; j < r; ++j) a += Bm[(int64_t)o * r + j] * A[(int64_t)j * in + k];
    dst[i] = W[i] + s * a;
}

// keep-mask of the LoRA dropout (common.h: drop_scale) as fp32, for vl_dropout_mask
__global__ void dropout_mask_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint32_t stream, float p,
                                    float inv_keep) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = drop_scale(seed, stream, (uint64_t)i, p, inv_keep);
}

}  // namespace

// ---------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------
void k_ce_loss(const float* logits, const int64_t* labels, int B, int C, float* dlogits, float* loss_img, float* loss,
               int* err, hipStream_t s) {
    hipLaunchKernelGGL(ce_loss_kernel, dim3((B + 3) / 4), dim3(256), 0, s, logits, labels, B, C, dlogits, loss_img, err);
    hipLaunchKernelGGL(ce_reduce_kernel, dim3(1), dim3(256), 0, s, loss_img, B, loss);
}
void k_grad_scale(const float* dlogits, int B, int C, int uniform, float* gscale, float* inv_gscale, hipStream_t s) {
    hipLaunchKernelGGL(grad_scale_kernel, dim3(uniform ? 1 : (B + 3) / 4), dim3(256), 0, s, dlogits, B, C, uniform, gscale, inv_gscale);
}
void k_classifier_grad(const float* dlogits, const float* xf, int B, int D, int C, float* dW, float* db, hipStream_t s) {
    hipLaunchKernelGGL(classifier_grad_kernel, dim3(nblk((int64_t)C * D, 256)), dim3(256), 0, s, dlogits, xf, B, D, C,
                       dW, db);
}
void k_pgd_step(float* adv, const float* x0, const float* grad, float eps, float alpha, float lo, float hi, int64_t n,
                hipStream_t s, int* err) {
    ProfScope prof_("pgd_step_kernel", 0.0, (double)n * 16.0, s);
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(pgd_step_kernel, dim3(nblk(n4 > 0 ? (n4 + 1) / 2 : 1, 256, 8192)), dim3(256), 0, s, adv, x0, grad, eps,
                       alpha, lo, hi, n4, n, err);
}
void k_zero(void* p, size_t bytes, hipStream_t s) {
    ProfScope prof_("zero_kernel", 0.0, (double)bytes, s);
    const int64_t n16 = (int64_t)(bytes / 16);
    if (n16 > 0) hipLaunchKernelGGL(zero_kernel, dim3(nblk(n16, 256, 4096)), dim3(256), 0, s, (f32x4*)p, n16);
}
void k_pgd_init(float* adv, const float* x0, float eps, float lo, float hi, uint64_t seed, int64_t n, hipStream_t s) {
    ProfScope prof_("pgd_init_kernel", 0.0, (double)n * 8.0, s);
    hipLaunchKernelGGL(pgd_init_kernel, dim3(nblk(n, 256, 4096)), dim3(256), 0, s, adv, x0, eps, lo, hi, seed, n);
}
void apgd_schedule_constants(int N, int* k0, int* kmin, int* dec) {
    *k0 = std::max((int)(0.22 * N), 1); *kmin = std::max((int)(0.06 * N), 1); *dec = std::max((int)(0.03 * N), 1);
}
void k_apgd_sched(ApgdSched* sched, int32_t* ctr, int N, hipStream_t s) {
    int k0, kmin, dec;
    apgd_schedule_constants(N, &k0, &kmin, &dec);
    hipLaunchKernelGGL(apgd_sched_kernel, dim3(1), dim3(64), 0, s, sched, ctr, N, k0, kmin, dec);
}
void k_apgd_rand_init(float* x_adv, const float* x0, float eps, uint64_t seed, int B, int64_t n_img, hipStream_t s) {
    ProfScope prof_("apgd_rand_init_kernel", 0.0, (double)B * n_img * 8.0, s);
    hipLaunchKernelGGL(apgd_rand_init_kernel, dim3(B), dim3(256), 0, s, x_adv, x0, eps, seed, n_img);
}
void k_apgd_start(float* x_adv, const float* src, int64_t n, hipStream_t s) {
    ProfScope prof_("apgd_start_kernel", 0.0, (double)n * 8.0, s);
    hipLaunchKernelGGL(apgd_start_kernel, dim3(nblk(n, 256, 4096)), dim3(256), 0, s, x_adv, src, n);
}
void k_apgd_track(const ApgdState& st, const float* loss_img, const float* logits, const int64_t* labels, int B, int C, int N,
                  float eps, float rho, hipStream_t s) {
    ProfScope prof_("apgd_track_kernel", 0.0, (double)B * (C + 16) * 4.0, s);
    hipLaunchKernelGGL(apgd_track_kernel, dim3((B + 3) / 4), dim3(256), 0, s, st, loss_img, logits, labels, B, C, N, eps, rho);
}
void k_apgd_step(float* x_adv, float* x_old, float* x_best, float* x_best_adv, float* grad_best, const float* x0,
                 const float* grad, const uint32_t* flags, const float* step, int B, int64_t n_img, float eps,
                 const ApgdSched* sched, int32_t* ctr, int N, float a, int last, hipStream_t s, int* err) {
    ProfScope prof_("apgd_step_kernel", 0.0, (double)B * n_img * 24.0, s);
    const int64_t n4 = n_img / 4;                    // n_img % 4 == 0 is the caller's to check
    const int per_img = nblk((n4 + 1) / 2, 256, std::max(1, 8192 / B));
    hipLaunchKernelGGL(apgd_step_kernel, dim3(per_img, B), dim3(256), 0, s, x_adv, x_old, x_best, x_best_adv, grad_best, x0, grad,
                       flags, step, n4, eps, sched, ctr, N, a, last, err);
}
void k_dlr_targeted_loss(const float* logits, const int64_t* labels, const int32_t* targets, int B, int C, float* dlogits,
                         float* loss_img, float* loss, int* err, hipStream_t s) {
    hipLaunchKernelGGL(dlr_targeted_loss_kernel, dim3((B + 3) / 4), dim3(256), 0, s, logits, labels, targets, B, C, dlogits, loss_img, err);
    if (loss) hipLaunchKernelGGL(ce_reduce_kernel, dim3(1), dim3(256), 0, s, loss_img, B, loss);
}
void k_apgd_targets(const float* logits, const int64_t* labels, int B, int C, int n_target, int32_t* targets,
                    int32_t* clean_correct, hipStream_t s) {
    hipLaunchKernelGGL(apgd_targets_kernel, dim3((B + 3) / 4), dim3(256), 0, s, logits, labels, B, C, n_target, targets, clean_correct);
}
void k_apgdt_fold(float* x_out, const float* x_best_adv, const int32_t* still_in, int32_t* still_out, const int32_t* run_robust,
                  int32_t* fooled_by, int run, int B, int64_t n_img, hipStream_t s) {
    ProfScope prof_("apgdt_fold_kernel", 0.0, (double)B * n_img * 8.0, s);
    const int64_t n4 = n_img / 4;                    // n_img % 4 == 0 is the caller's to check
    hipLaunchKernelGGL(apgdt_fold_kernel, dim3(nblk(n4, 256, std::max(1, 8192 / B)), B), dim3(256), 0, s, x_out, x_best_adv, still_in,
                       still_out, run_robust, fooled_by, run, n4);
}
// p = p_init / 2^k for the k thresholds that it = int((j - 1) / N * 10000) exceeds strictly; side = round-half-even(sqrt(p S S)),
// all in double (p_init enters as the float the ABI carries).  from[k] = the first proposal that uses side[k], N + 1 if none.
void square_schedule(int S, int N, float p_init, SquareSched* out) {
    static const int thr[9] = {10, 50, 200, 500, 1000, 2000, 4000, 6000, 8000};
    for (int i = 0; i < 10; ++i) {
        const double p = (double)p_init / (double)(1 << i);
        const double v = std::nearbyint(std::sqrt(p * S * S));
        out->side[i] = std::min(S, std::max(1, (int)v));
        out->from[i] = N + 1;
    }
    for (int j = N; j >= 1; --j) {
        const int it = (int)((double)(j - 1) / (double)N * 10000.0);
        int k = 0;
        for (int i = 0; i < 9; ++i) k += it > thr[i] ? 1 : 0;
        out->from[k] = j;
    }
    out->from[0] = 1;
    for (int i = 8; i >= 1; --i) out->from[i] = std::min(out->from[i], out->from[i + 1]);     // a k the schedule jumps over
}
void k_square_sched(const SquareState& st, const SquareSched& sc, int N, uint64_t seed, uint64_t image_offset, hipStream_t s) {
    hipLaunchKernelGGL(square_sched_kernel, dim3(1), dim3(256), 0, s, st, sc, N, seed, image_offset);
}
void k_square_init(float* x_cur, float* x_best, const float* x0, const SquareParams* par, int B, int S, float eps, hipStream_t s) {
    ProfScope prof_("square_init_kernel", 0.0, (double)B * 3 * S * S * 12.0, s);
    hipLaunchKernelGGL(square_init_kernel, dim3(nblk((int64_t)3 * S * S, 256, std::max(1, 4096 / B)), B), dim3(256), 0, s, x_cur,
                       x_best, x0, par, S, eps);
}
void k_square_track(const SquareState& st, const float* logits, const int64_t* labels, int B, int C, int S, int N, hipStream_t s,
                    int* err) {
    ProfScope prof_("square_track_kernel", 0.0, (double)B * (C + 24) * 4.0, s);
    hipLaunchKernelGGL(square_track_kernel, dim3((B + 3) / 4), dim3(256), 0, s, st, logits, labels, B, C, S, N, err);
}
void k_square_step(float* x_cur, float* x_best, const float* x0, const uint32_t* flags, const int32_t* win_prev,
                   const int32_t* win_next, int B, int S, float eps, int32_t* ctr, int N, hipStream_t s) {
    ProfScope prof_("square_step_kernel", 0.0, 0.0, s);      // the traffic depends on the windows: 3 (s_prev^2 + s_next^2) x 12 B at most
    // the grid is fixed at capture for the largest pair of windows (4 items per thread there); later, smaller windows leave
    // most blocks with nothing to do
    const int per_img = nblk((int64_t)6 * S * S, 1024, std::max(1, 2048 / B));
    hipLaunchKernelGGL(square_step_kernel, dim3(per_img, B), dim3(256), 0, s, x_cur, x_best, x0, flags, win_prev, win_next, S, eps,
                       ctr, N);
}
void k_adam(float* p, const float* g, float* m, float* v, float lr, float b1, float b2, float eps, int t, int64_t n,
            hipStream_t s, int* err) {
    ProfScope prof_("adam_kernel", 0.0, (double)n * 28.0, s);
    const float bc1 = 1.f - powf(b1, (float)t);
    const float sqrt_bc2 = sqrtf(1.f - powf(b2, (float)t));
    hipLaunchKernelGGL(adam_kernel, dim3(nblk(n, 256)), dim3(256), 0, s, p, g, m, v, lr, b1, b2, eps, bc1, sqrt_bc2, n, err);
}
void k_channel_affine(float* dst, const float* src, const float* scale, const float* shift, int B, int64_t hw,
                      hipStream_t s) {
    const int64_t n = (int64_t)B * 3 * hw;
    hipLaunchKernelGGL(channel_affine_kernel, dim3(nblk(n, 256, 4096)), dim3(256), 0, s, dst, src, scale[0], scale[1],
                       scale[2], shift[0], shift[1], shift[2], hw, n);
}
void k_quantize(const float* img, uint8_t* out, int B, int C, int H, int W, hipStream_t s) {
    const int64_t n = (int64_t)B * C * H * W;
    hipLaunchKernelGGL(quantize_kernel, dim3(nblk(n, 256)), dim3(256), 0, s, img, out, B, C, H, W);
}
void k_merge_f32(const float* W, const float* A, const float* B, int out, int in, int r, float sc, float* dst,
                 hipStream_t s) {
    const int64_t n = (int64_t)out * in;
    hipLaunchKernelGGL(merge_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, W, A, B, out, in, r, sc, dst);
}
void k_dropout_mask(float* out, int64_t n, uint64_t seed, uint32_t stream, float p, hipStream_t s) {
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(nblk(n, 256, 4096)), dim3(256), 0, s, out, n, seed, stream, p,
                       1.f / (1.f - p));
}

}  // namespace vl_once
