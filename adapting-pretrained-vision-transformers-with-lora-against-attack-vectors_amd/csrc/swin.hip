// Swin Transformer (Swin-T by default) + LoRA forward / backward-to-input / PGD behind the vl_swin_* C ABI
// (BASELINE config 4; the reference lists Swin-T in README.md:53 but holds no code for it: the oracle is HF's
// SwinForImageClassification built from a local SwinConfig, modeling_swin.py).  fp32 throughout: the GEMMs run on the
// exact-f32 MFMA kernel of the parity mode (f32_kernels.hip), the windowed attention below is a HIP kernel of its own:
//   * window partition, cyclic shift and their inverses are pure INDEX arithmetic inside the attention kernels
//     (token p of window w of the rolled image -> row of the [B, H*W, C] activation), nothing is copied or rolled;
//   * the shift mask (-100 between different regions, SwinLayer.get_attn_mask) and the relative position bias
//     (table[(dy+6)*13 + (dx+6)][head]) are evaluated on the fly;
//   * one wave per (image, window, head): lane = query (forward, dQ) or key (dK, dV); 49 tokens, head_dim 32.
// This is the functional first form of the path (parity first); an fp16 MFMA form of the window kernels is the next step.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/vitlora.h"
#include "f32_kernels.h"
#include "kernels.h"
#include "env.h"
#include "model.h"
#include "prof.h"

namespace VLNS {      // vl_f16 / vl_bf16: the 16-bit path is compiled once per operand type (common.h)

namespace {

constexpr int WS = 7, WT = 49, HDIM = 32, KLD = 33;
typedef _Float16 sh16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 sh16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int win_row(int b, int w, int p, int H, int W, int shift) {
    const int nwx = W / WS;
    int y = (w / nwx) * WS + p / WS + shift, x = (w % nwx) * WS + p % WS + shift;
    if (y >= H) y -= H;
    if (x >= W) x -= W;
    return (b * H + y) * W + x;
}
// region id of a position of the ROLLED image (SwinLayer.get_attn_mask): rows / columns >= H - 7 and >= H - shift
__device__ __forceinline__ int win_region(int w, int p, int H, int W, int shift) {
    const int nwx = W / WS;
    const int y = (w / nwx) * WS + p / WS, x = (w % nwx) * WS + p % WS;
    return ((y >= H - WS) + (y >= H - shift)) * 3 + (x >= W - WS) + (x >= W - shift);
}
__device__ __forceinline__ int bias_index(int pi, int pj) { return (pi / WS - pj / WS + WS - 1) * (2 * WS - 1) + (pi % WS - pj % WS + WS - 1); }

// ---------------------------------------------------------------------------------------------------------------
// forward: ctx = softmax(q k^T / sqrt(32) + bias + mask) v per (image, window, head)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void win_attn_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                           float* __restrict__ ctx, float* __restrict__ lse, int B, int H, int W,
                                                           int C, int heads, int shift) {
    __shared__ float sK[4][WT * KLD], sV[4][WT * KLD];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nW = (H / WS) * (W / WS);
    const int64_t item = (int64_t)blockIdx.x * 4 + wv;
    if (item >= (int64_t)B * nW * heads) return;
    const int hd = (int)(item % heads);
    const int w = (int)((item / heads) % nW);
    const int b = (int)(item / ((int64_t)heads * nW));
    const int p = lane < WT ? lane : WT - 1;
    const int row = win_row(b, w, p, H, W, shift);
    const float* src = qkv + (int64_t)row * 3 * C + hd * HDIM;
    float q[HDIM];
#pragma unroll
    for (int d = 0; d < HDIM; d += 4) {
        const f32x4 a = *(const f32x4*)(src + d), k4 = *(const f32x4*)(src + C + d), v4 = *(const f32x4*)(src + 2 * C + d);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            q[d + e] = a[e];
            if (lane < WT) { sK[wv][p * KLD + d + e] = k4[e]; sV[wv][p * KLD + d + e] = v4[e]; }
        }
    }
    __builtin_amdgcn_wave_barrier();
    const int reg_i = shift ? win_region(w, p, H, W, shift) : 0;
    float s[WT], mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < WT; ++j) {
        float a = 0.f;
#pragma unroll
        for (int d = 0; d < HDIM; ++d) a = fmaf(q[d], sK[wv][j * KLD + d], a);
        a = a * 0.17677669529663687f + table[bias_index(p, j) * heads + hd];
        if (shift && win_region(w, j, H, W, shift) != reg_i) a += -100.0f;
        s[j] = a;
        mx = fmaxf(mx, a);
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < WT; ++j) { s[j] = expf(s[j] - mx); sum += s[j]; }
    const float inv = 1.f / sum;
    float o[HDIM];
#pragma unroll
    for (int d = 0; d < HDIM; ++d) o[d] = 0.f;
#pragma unroll
    for (int j = 0; j < WT; ++j) {
        const float pj = s[j] * inv;
#pragma unroll
        for (int d = 0; d < HDIM; ++d) o[d] = fmaf(pj, sV[wv][j * KLD + d], o[d]);
    }
    if (lane < WT) {
        float* dst = ctx + (int64_t)row * C + hd * HDIM;
#pragma unroll
        for (int d = 0; d < HDIM; d += 4) *(f32x4*)(dst + d) = f32x4{o[d], o[d + 1], o[d + 2], o[d + 3]};
        lse[(int64_t)row * heads + hd] = mx + logf(sum);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// backward: dq (lane = query), then dk, dv (lane = key); P recomputed from the saved log-sum-exp
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void win_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                           const float* __restrict__ ctx, const float* __restrict__ dctx,
                                                           const float* __restrict__ lse, float* __restrict__ dqkv, int B, int H,
                                                           int W, int C, int heads, int shift) {
    __shared__ float sQ[2][WT * KLD], sK[2][WT * KLD], sV[2][WT * KLD], sdO[2][WT * KLD], sL[2][64], sD[2][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nW = (H / WS) * (W / WS);
    const int64_t item = (int64_t)blockIdx.x * 2 + wv;
    if (item >= (int64_t)B * nW * heads) return;
    const int hd = (int)(item % heads);
    const int w = (int)((item / heads) % nW);
    const int b = (int)(item / ((int64_t)heads * nW));
    const int p = lane < WT ? lane : WT - 1;
    const int row = win_row(b, w, p, H, W, shift);
    const float* src = qkv + (int64_t)row * 3 * C + hd * HDIM;
    const float* dsrc = dctx + (int64_t)row * C + hd * HDIM;
    const float* osrc = ctx + (int64_t)row * C + hd * HDIM;
    float a_[HDIM], b_[HDIM];          // pass 1: q_i, dO_i ; pass 2: k_j, v_j
    float delta = 0.f;
#pragma unroll
    for (int d = 0; d < HDIM; d += 4) {
        const f32x4 q4 = *(const f32x4*)(src + d), k4 = *(const f32x4*)(src + C + d), v4 = *(const f32x4*)(src + 2 * C + d);
        const f32x4 g4 = *(const f32x4*)(dsrc + d), o4 = *(const f32x4*)(osrc + d);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a_[d + e] = q4[e]; b_[d + e] = g4[e];
            delta = fmaf(g4[e], o4[e], delta);
            if (lane < WT) {
                sQ[wv][p * KLD + d + e] = q4[e]; sK[wv][p * KLD + d + e] = k4[e];
                sV[wv][p * KLD + d + e] = v4[e]; sdO[wv][p * KLD + d + e] = g4[e];
            }
        }
    }
    const float lse_i = lse[(int64_t)row * heads + hd];
    if (lane < WT) { sL[wv][p] = lse_i; sD[wv][p] = delta; }
    __builtin_amdgcn_wave_barrier();
    const int reg_p = shift ? win_region(w, p, H, W, shift) : 0;
    const float scale = 0.17677669529663687f;
    // ---- pass 1: lane = query i ----
    float acc[HDIM];
#pragma unroll
    for (int d = 0; d < HDIM; ++d) acc[d] = 0.f;
    for (int j = 0; j < WT; ++j) {
        float sdot = 0.f, dp = 0.f;
#pragma unroll
        for (int d = 0; d < HDIM; ++d) { sdot = fmaf(a_[d], sK[wv][j * KLD + d], sdot); dp = fmaf(b_[d], sV[wv][j * KLD + d], dp); }
        float sc = sdot * scale + table[bias_index(p, j) * heads + hd];
        if (shift && win_region(w, j, H, W, shift) != reg_p) sc += -100.0f;
        const float pr = expf(sc - lse_i);
        const float ds = pr * (dp - delta) * scale;
#pragma unroll
        for (int d = 0; d < HDIM; ++d) acc[d] = fmaf(ds, sK[wv][j * KLD + d], acc[d]);
    }
    float* dst = dqkv + (int64_t)row * 3 * C + hd * HDIM;
    if (lane < WT) {
#pragma unroll
        for (int d = 0; d < HDIM; d += 4) *(f32x4*)(dst + d) = f32x4{acc[d], acc[d + 1], acc[d + 2], acc[d + 3]};
    }
    // ---- pass 2: lane = key j ----
#pragma unroll
    for (int d = 0; d < HDIM; ++d) { a_[d] = sK[wv][p * KLD + d]; b_[d] = sV[wv][p * KLD + d]; }
    float dk[HDIM], dv[HDIM];
#pragma unroll
    for (int d = 0; d < HDIM; ++d) { dk[d] = 0.f; dv[d] = 0.f; }
    for (int i = 0; i < WT; ++i) {
        float sdot = 0.f, dp = 0.f;
#pragma unroll
        for (int d = 0; d < HDIM; ++d) { sdot = fmaf(sQ[wv][i * KLD + d], a_[d], sdot); dp = fmaf(sdO[wv][i * KLD + d], b_[d], dp); }
        float sc = sdot * scale + table[bias_index(i, p) * heads + hd];
        if (shift && win_region(w, i, H, W, shift) != reg_p) sc += -100.0f;
        const float pr = expf(sc - sL[wv][i]);
        const float ds = pr * (dp - sD[wv][i]) * scale;
#pragma unroll
        for (int d = 0; d < HDIM; ++d) { dk[d] = fmaf(ds, sQ[wv][i * KLD + d], dk[d]); dv[d] = fmaf(pr, sdO[wv][i * KLD + d], dv[d]); }
    }
    if (lane < WT) {
#pragma unroll
        for (int d = 0; d < HDIM; d += 4) {
            *(f32x4*)(dst + C + d) = f32x4{dk[d], dk[d + 1], dk[d + 2], dk[d + 3]};
            *(f32x4*)(dst + 2 * C + d) = f32x4{dv[d], dv[d + 1], dv[d + 2], dv[d + 3]};
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// patch embedding gather (Conv2d k = s = P as a GEMM), patch merging gather / scatter, mean-pool head
// ---------------------------------------------------------------------------------------------------------------
// merged[b, (y/2)*(W/2) + x/2, q*C + c] = x[b, y, x, c], q = (x & 1) * 2 + (y & 1)   (SwinPatchMerging.forward: col-major quad order)
__global__ void merge_gather_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int H, int W, int C, int inverse) {
    const int64_t total = (int64_t)B * H * W * C;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += stride) {
        const int c = (int)(t % C);
        int64_t r = t / C;
        const int xx = (int)(r % W); r /= W;
        const int yy = (int)(r % H);
        const int b = (int)(r / H);
        const int64_t m = ((int64_t)b * (H / 2) + yy / 2) * (W / 2) + xx / 2;
        const int64_t o = m * 4 * C + ((xx & 1) * 2 + (yy & 1)) * C + c;
        if (inverse) out[t] = x[o]; else out[o] = x[t];
    }
}
// 16-bit path: SwinPatchMerging's {2x2 gather, LayerNorm(4C)} in ONE pass over the stage output, which is read where it lies
// (the fp32 stream xb of the stage's last block + that block's h16 MLP output `delta`, row stride ldd): no materialised stage
// output, no gathered copy, no fp32 LayerNorm output, no pack pass -- the normalised rows leave as the h16 A operand of the
// reduction GEMM.  Row r of the merged map = (b, y2, x2); its 4C features are C float4 chunks: chunk c belongs to quadrant
// q = c / (C/4) = (x & 1) * 2 + (y & 1) (merge_gather_kernel's order).  NV chunks per lane, G lanes per row.
template <int NV, int G>
__global__ __launch_bounds__(256) void merge_ln_fwd16_kernel(const h16* __restrict__ xb, const h16* __restrict__ delta, int ldd,
                                                             h16* __restrict__ out, float* __restrict__ mean_out,
                                                             float* __restrict__ rstd_out, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, int B, int H, int W, int C, float eps) {
    const int lane = threadIdx.x & 63, li = lane % G;
    const int64_t Mq = (int64_t)B * (H / 2) * (W / 2);
    const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / G) + lane / G;
    const bool live = row < Mq;
    const int64_t r = live ? row : Mq - 1;
    const int x2 = (int)(r % (W / 2)), y2 = (int)((r / (W / 2)) % (H / 2)), b = (int)(r / ((int64_t)(W / 2) * (H / 2)));
    const int cq = C >> 2;                     // float4 chunks per quadrant
    f32x4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = li + i * G, q = c / cq, ci = c - q * cq;
        const int64_t src = ((int64_t)b * H + 2 * y2 + (q & 1)) * W + 2 * x2 + (q >> 1);
        const sh16x4 a = *(const sh16x4*)(xb + src * C + ci * 4);
        const sh16x4 d = *(const sh16x4*)(delta + src * ldd + ci * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[i][k] = (float)f2h((float)a[k] + (float)d[k]); s += v[i][k]; }      // x' = round16(xb + delta): the stream value
    }
    const float D = 4.f * C;
    float mean = s, qs = 0.f;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) mean += __shfl_xor(mean, o, 64);
    mean /= D;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float t = v[i][k] - mean; qs += t * t; }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) qs += __shfl_xor(qs, o, 64);
    const float rstd = 1.0f / sqrtf(qs / D + eps);
    if (!live) return;
    if (li == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = li + i * G;
        const f32x4 g = *(const f32x4*)(gamma + c * 4), bb = *(const f32x4*)(beta + c * 4);
        sh16x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = f2h((v[i][k] - mean) * rstd * g[k] + bb[k]);
        *(sh16x4*)(out + row * 4 * C + c * 4) = o;
    }
}
// ... and its backward: dy [Mq, 4C] fp32 (the reduction's dgrad), x gathered again from xb + delta; the gradient w.r.t. the
// stage output is scattered straight to its rows, as fp32 (residual-gradient stream) and h16 (row stride ldh)
template <int NV, int G>
__global__ __launch_bounds__(256) void merge_ln_bwd16_kernel(const h16* __restrict__ dy, const h16* __restrict__ xb,
                                                             const h16* __restrict__ delta, int ldd, const float* __restrict__ mean_in,
                                                             const float* __restrict__ rstd_in, const float* __restrict__ gamma,
                                                             h16* __restrict__ dx_h, int ldh, int B, int H, int W,
                                                             int C, int* __restrict__ err) {
    const int lane = threadIdx.x & 63, li = lane % G;
    const int64_t Mq = (int64_t)B * (H / 2) * (W / 2);
    const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / G) + lane / G;
    const bool live = row < Mq;
    const int64_t r = live ? row : Mq - 1;
    const int x2 = (int)(r % (W / 2)), y2 = (int)((r / (W / 2)) % (H / 2)), b = (int)(r / ((int64_t)(W / 2) * (H / 2)));
    const int cq = C >> 2;
    const float mean = mean_in[r], rstd = rstd_in[r];
    f32x4 g[NV], xh[NV];
    int64_t srow[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = li + i * G, q = c / cq, ci = c - q * cq;
        srow[i] = (((int64_t)b * H + 2 * y2 + (q & 1)) * W + 2 * x2 + (q >> 1));
        const sh16x4 a = *(const sh16x4*)(xb + srow[i] * C + ci * 4);
        const sh16x4 d = *(const sh16x4*)(delta + srow[i] * ldd + ci * 4);
        const sh16x4 dv = *(const sh16x4*)(dy + r * 4 * C + c * 4);
        const f32x4 gm = *(const f32x4*)(gamma + c * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            g[i][k] = (float)dv[k] * gm[k];
            // (the forward normalised the ROUNDED sum: the merge reads x' = round16(xb + delta) where the blocks keep it)
            xh[i][k] = ((float)f2h((float)a[k] + (float)d[k]) - mean) * rstd;
            s1 += g[i][k];
            s2 += g[i][k] * xh[i][k];
        }
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    const float c1 = s1 / (4.f * C), c2 = s2 / (4.f * C);
    if (!live) return;
    bool sat = false;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = li + i * G, q = c / cq, ci = c - q * cq;
        f32x4 o; sh16x4 ob;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k] = rstd * (g[i][k] - c1 - xh[i][k] * c2);
            ob[k] = f2h_sat(o[k]);
            sat |= !(fabsf(o[k]) <= 65504.f);
        }
        *(sh16x4*)(dx_h + srow[i] * ldh + ci * 4) = ob;
    }
    // pad columns of the four un-merged rows (row stride ldh > C): zeros -- the next dgrad GEMM reads them against zero weights
    const int pc = (ldh - C) >> 2;
    for (int idx = li; idx < 4 * pc; idx += G) {
        const int q = idx / pc, ci = idx - q * pc;
        const int64_t sr = (((int64_t)b * H + 2 * y2 + (q & 1)) * W + 2 * x2 + (q >> 1));
        *(sh16x4*)(dx_h + sr * ldh + C + ci * 4) = sh16x4{0, 0, 0, 0};
    }
    if (sat && err) *err = 2;
}
// C = 96: 3 chunks x 32 lanes (two rows per wave); 192: 3 x 64; 384: 6 x 64
template <class F> inline bool merge_dispatch(int C, F&& f) {
    if (C == 96) { f(std::integral_constant<int, 3>{}, std::integral_constant<int, 32>{}); return true; }
    if (C == 192) { f(std::integral_constant<int, 3>{}, std::integral_constant<int, 64>{}); return true; }
    if (C == 384) { f(std::integral_constant<int, 6>{}, std::integral_constant<int, 64>{}); return true; }
    return false;
}

// ---------------------------------------------------------------------------------------------------------------
// 16-bit residual streams of the Swin path (round 5; the ViT path got them in round 4, elementwise.hip): the stream x and its
// gradient are h16 tensors, a LayerNorm pass moves 8 B per element instead of 12 (forward) / 16 (backward).
//   forward   x' = round16(x + delta) (delta optional: the h16 output of the projection before it), h = LN(x'); either output
//             optional; statistics fp32; XF32: x is an fp32 tensor (the patch embedding's output)
//   backward  g <- g + LN'(dh)  IN PLACE (gres == gout allowed): the stream gradient is also the A operand of the next dgrad
//             GEMM; XF32 / OF32: fp32 x / fp32 output (the embedding LayerNorm at the bottom of the network)
// LPR lanes per row (16: rows of <= 128 elements, four rows per wave; 32: two rows per wave), NV 16-byte chunks per lane.
// Rows may be padded (row strides > D): the pad columns of h and of the gradient stream are WRITTEN with zeros by these kernels
// -- they meet zero weight columns in the next GEMM, so a workspace need not be zeroed at hand-over for them (round-4 verdict 8).
// ---------------------------------------------------------------------------------------------------------------
template <int LPR> __device__ __forceinline__ float seg_sum(float v) {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int NV, int LPR, bool XF32>
__global__ __launch_bounds__(256) void sw_ln_fwd16_kernel(const void* __restrict__ xin, int ldx, const h16* __restrict__ delta, int ldd,
                                                          h16* __restrict__ xout, int ldo, h16* __restrict__ h, int ldh,
                                                          float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, int M, int D,
                                                          float eps, int* __restrict__ err) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, li = lane % LPR, seg = lane / LPR;
    const int nc = D >> 3;
    const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + seg;
    const bool live = row < M;
    const int64_t r = live ? row : M - 1;
    f32x4 v[NV][2];
    float s = 0.f;
    bool sat = false;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = li + i * LPR;
        v[i][0] = v[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < nc) {
            if constexpr (XF32) {
                const float* xp = (const float*)xin + r * ldx + c * 8;
                v[i][0] = *(const f32x4*)xp; v[i][1] = *(const f32x4*)(xp + 4);
            } else {
                const sh16x8 xv = *(const sh16x8*)((const h16*)xin + r * ldx + c * 8);
#pragma unroll
                for (int k = 0; k < 8; ++k) v[i][k >> 2][k & 3] = (float)xv[k];
            }
            if (delta) {
                const sh16x8 dl = *(const sh16x8*)(delta + r * ldd + c * 8);
#pragma unroll
                for (int k = 0; k < 8; ++k) v[i][k >> 2][k & 3] += (float)dl[k];
            }
            if (delta) {      // the stream holds the ROUNDED sum: the backward re-derives xhat from it
                sh16x8 xr;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float a = v[i][k >> 2][k & 3];
                    sat |= !(fabsf(a) <= 65504.f);
                    xr[k] = f2h(a);
                    v[i][k >> 2][k & 3] = (float)xr[k];
                }
                if (xout && live) *(sh16x8*)(xout + r * ldo + c * 8) = xr;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) s += v[i][0][k] + v[i][1][k];
        }
    }
    if (!h) { if (sat && err) *err = 4; return; }
    const float mean = seg_sum<LPR>(s) / D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
        if (li + i * LPR < nc) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { const float d0 = v[i][0][k] - mean, d1 = v[i][1][k] - mean; q += d0 * d0 + d1 * d1; }
        }
    const float rstd = rsqrtf(seg_sum<LPR>(q) / D + eps);
    if (live) {
        if (li == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = li + i * LPR;
            if (c < nc) {
                const f32x4 g0 = *(const f32x4*)(gamma + c * 8), g1 = *(const f32x4*)(gamma + c * 8 + 4);
                const f32x4 b0 = *(const f32x4*)(beta + c * 8), b1 = *(const f32x4*)(beta + c * 8 + 4);
                sh16x8 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    o[k] = f2h((v[i][0][k] - mean) * rstd * g0[k] + b0[k]);
                    o[4 + k] = f2h((v[i][1][k] - mean) * rstd * g1[k] + b1[k]);
                }
                *(sh16x8*)(h + r * ldh + c * 8) = o;
            }
        }
        const sh16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int c = nc + li; c < (ldh >> 3); c += LPR) *(sh16x8*)(h + r * ldh + c * 8) = z;      // pad columns
    }
    if (sat && err) *err = 4;
}

// gout = gres + rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dh * gamma, xhat = (x - mean) * rstd
template <int NV, int LPR, bool XF32, bool OF32>
__global__ __launch_bounds__(256) void sw_ln_bwd16_kernel(const h16* __restrict__ dh, int ldd, const void* __restrict__ xin, int ldx,
                                                          const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                          const float* __restrict__ gamma, const h16* gres, void* gout, int ldg,
                                                          int M, int D, int* __restrict__ err) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, li = lane % LPR, seg = lane / LPR;
    const int nc = D >> 3;
    const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + seg;
    const bool live = row < M;
    const int64_t r = live ? row : M - 1;
    const float mean = mean_in[r], rstd = rstd_in[r];
    f32x4 g[NV][2], xh[NV][2];
    sh16x8 rv[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = li + i * LPR;
        g[i][0] = g[i][1] = xh[i][0] = xh[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        rv[i] = sh16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (c < nc) {
            const sh16x8 d = *(const sh16x8*)(dh + r * ldd + c * 8);
            f32x4 x0, x1;
            if constexpr (XF32) {
                const float* xp = (const float*)xin + r * ldx + c * 8;
                x0 = *(const f32x4*)xp; x1 = *(const f32x4*)(xp + 4);
            } else {
                const sh16x8 xv = *(const sh16x8*)((const h16*)xin + r * ldx + c * 8);
#pragma unroll
                for (int k = 0; k < 4; ++k) { x0[k] = (float)xv[k]; x1[k] = (float)xv[4 + k]; }
            }
            if (gres) rv[i] = *(const sh16x8*)(gres + r * ldg + c * 8);
            const f32x4 g0 = *(const f32x4*)(gamma + c * 8), g1 = *(const f32x4*)(gamma + c * 8 + 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                g[i][0][k] = (float)d[k] * g0[k];
                g[i][1][k] = (float)d[4 + k] * g1[k];
                xh[i][0][k] = (x0[k] - mean) * rstd;
                xh[i][1][k] = (x1[k] - mean) * rstd;
                s1 += g[i][0][k] + g[i][1][k];
                s2 += g[i][0][k] * xh[i][0][k] + g[i][1][k] * xh[i][1][k];
            }
        }
    }
    const float c1 = seg_sum<LPR>(s1) / D, c2 = seg_sum<LPR>(s2) / D;
    if (!live) return;
    bool sat = false;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = li + i * LPR;
        if (c < nc) {
            float o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                o[k] = (float)rv[i][k] + rstd * (g[i][k >> 2][k & 3] - c1 - xh[i][k >> 2][k & 3] * c2);
                sat |= !(fabsf(o[k]) <= 65504.f);
            }
            if constexpr (OF32) {
                float* op = (float*)gout + r * ldg + c * 8;
                *(f32x4*)op = f32x4{o[0], o[1], o[2], o[3]};
                *(f32x4*)(op + 4) = f32x4{o[4], o[5], o[6], o[7]};
            } else {
                sh16x8 ob;
#pragma unroll
                for (int k = 0; k < 8; ++k) ob[k] = f2h_sat(o[k]);
                *(sh16x8*)((h16*)gout + r * ldg + c * 8) = ob;
            }
        }
    }
    if constexpr (!OF32) {
        const sh16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int c = nc + li; c < (ldg >> 3); c += LPR) *(sh16x8*)((h16*)gout + r * ldg + c * 8) = z;      // pad columns
    }
    if (sat && err && !OF32) *err = 2;
}

// launchers: D in {96, 192, 384, 768} (and any D % 8 == 0 up to 768)
template <bool XF32>
void sw_ln_fwd16(const void* x, int ldx, const h16* delta, int ldd, h16* xout, int ldo, h16* h, int ldh, float* mean, float* rstd,
                 const float* g, const float* b, int M, int D, float eps, int* err, hipStream_t s) {
    const int nc = D / 8;
#define SWF(NV_, LPR_) hipLaunchKernelGGL((sw_ln_fwd16_kernel<NV_, LPR_, XF32>), dim3((M + 4 * (64 / LPR_) - 1) / (4 * (64 / LPR_))), dim3(256), 0, s, \
                                          x, ldx, delta, ldd, xout, ldo, h, ldh, mean, rstd, g, b, M, D, eps, err)
    if (nc <= 16) SWF(1, 16); else if (nc <= 32) SWF(1, 32); else if (nc <= 64) SWF(2, 32); else SWF(3, 32);
#undef SWF
}
template <bool XF32, bool OF32>
void sw_ln_bwd16(const h16* dh, int ldd, const void* x, int ldx, const float* mean, const float* rstd, const float* g, const h16* gres,
                 void* gout, int ldg, int M, int D, int* err, hipStream_t s) {
    const int nc = D / 8;
#define SWB(NV_, LPR_) hipLaunchKernelGGL((sw_ln_bwd16_kernel<NV_, LPR_, XF32, OF32>), dim3((M + 4 * (64 / LPR_) - 1) / (4 * (64 / LPR_))), dim3(256), 0, s, \
                                          dh, ldd, x, ldx, mean, rstd, g, gres, gout, ldg, M, D, err)
    if (nc <= 16) SWB(1, 16); else if (nc <= 32) SWB(1, 32); else if (nc <= 64) SWB(2, 32); else SWB(3, 32);
#undef SWB
}

// 16-bit patch embedding of Swin (round 5; P = 4: a patch row is 4 pixels = one 16-byte fp32 load): pixels [B,3,S,S] f32 ->
// patches [B*G*G][3*P*P = 48] h16 with (x - mean) / std fused, 8 columns (two patch rows of one channel) per thread; and the way
// back: d(pixels)[b,c,y,x] = d(patches)[m][c*16 + ph*4 + pw] * inv_std[c] * unscale[b] (the per-image power-of-two gradient
// scale is undone here, not in a pass of its own over the 154 MB pixel gradient)
__global__ void patch_gather16_p4_kernel(const float* __restrict__ x, h16* __restrict__ out, int B, int S, int G, int normalise,
                                         float m0, float m1, float m2, float is0, float is1, float is2) {
    const int64_t total = (int64_t)B * G * G * 6, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += stride) {
        const int c8 = (int)(t % 6);
        const int64_t mrow = t / 6;
        const int c = c8 >> 1, ph = (c8 & 1) * 2;
        const int b = (int)(mrow / (G * G)), pi = (int)(mrow - (int64_t)b * G * G);
        const int py = pi / G, px = pi - py * G;
        const float* src = x + (((int64_t)b * 3 + c) * S + py * 4 + ph) * S + px * 4;
        const f32x4 v0 = *(const f32x4*)src, v1 = *(const f32x4*)(src + S);
        float mean = 0.f, is = 1.f;
        if (normalise) { mean = c == 0 ? m0 : (c == 1 ? m1 : m2); is = c == 0 ? is0 : (c == 1 ? is1 : is2); }
        sh16x8 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) { o[i] = f2h((v0[i] - mean) * is); o[4 + i] = f2h((v1[i] - mean) * is); }
        *(sh16x8*)(out + mrow * 48 + c8 * 8) = o;
    }
}
__global__ void patch_scatter16_p4_kernel(const h16* __restrict__ dp, float* __restrict__ gx, int B, int S, int G, float is0,
                                          float is1, float is2, const float* __restrict__ unscale, int* __restrict__ err) {
    const int64_t total = (int64_t)B * G * G * 6, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += stride) {
        const int c8 = (int)(t % 6);
        const int64_t mrow = t / 6;
        const int c = c8 >> 1, ph = (c8 & 1) * 2;
        const int b = (int)(mrow / (G * G)), pi = (int)(mrow - (int64_t)b * G * G);
        const int py = pi / G, px = pi - py * G;
        const sh16x8 v = *(const sh16x8*)(dp + mrow * 48 + c8 * 8);
        const float f = (c == 0 ? is0 : (c == 1 ? is1 : is2)) * (unscale ? unscale[b] : 1.f);
        f32x4 o0, o1;
#pragma unroll
        for (int i = 0; i < 4; ++i) { o0[i] = (float)v[i] * f; o1[i] = (float)v[4 + i] * f; }
        if (err && !(fabsf(o0[0]) < INFINITY && fabsf(o0[1]) < INFINITY && fabsf(o0[2]) < INFINITY && fabsf(o0[3]) < INFINITY &&
                     fabsf(o1[0]) < INFINITY && fabsf(o1[1]) < INFINITY && fabsf(o1[2]) < INFINITY && fabsf(o1[3]) < INFINITY)) *err = 2;
        float* dst = gx + (((int64_t)b * 3 + c) * S + py * 4 + ph) * S + px * 4;
        *(f32x4*)dst = o0;
        *(f32x4*)(dst + S) = o1;
    }
}

// The unpadded stages' h16 activations have rows NARROWER than the padded K of the GEMM that reads them: the last valid row's
// K tail is read from the first bytes of the row after it, against zero weight columns.  That row is never written (a pad row,
// or the 512-byte slack behind the buffer), so these 256-byte heads are zeroed at the start of every forward: 0 x garbage would
// be NaN.  With this and the pad-column writes of the LayerNorm / merge kernels the Swin workspace needs no zeroed hand-over
// (round-4 verdict 8; tests/test_hip_swin.py pre-fills it with 0xFF).
struct TailPtrs { h16* p[16]; int n; };
__global__ void zero_tails_kernel(TailPtrs t) {
    if ((int)blockIdx.x < t.n && threadIdx.x < 16) ((f32x4*)t.p[blockIdx.x])[threadIdx.x] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// mean pool over the L tokens of an h16 tensor, and its backward into an h16 gradient (the per-image gradient scale keeps it in range)
__global__ void mean_pool16_kernel(const h16* __restrict__ h, float* __restrict__ pooled, int B, int L, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C;
    float s = 0.f;
    for (int t = 0; t < L; ++t) s += (float)h[((int64_t)b * L + t) * C + c];
    pooled[i] = s / L;
}
__global__ void mean_pool_bwd16_kernel(const float* __restrict__ dpooled, h16* __restrict__ dh, int B, int L, int C) {
    const int64_t total = (int64_t)B * L * C;
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const int b = (int)(i / ((int64_t)L * C));
    dh[i] = f2h_sat(dpooled[b * C + c] / L);
}

// pooled[b][c] = mean over the L tokens of h[b][t][c]; inverse: dh[b][t][c] = dpooled[b][c] / L
__global__ void mean_pool_kernel(const float* __restrict__ h, float* __restrict__ pooled, int B, int L, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C;
    float s = 0.f;
    for (int t = 0; t < L; ++t) s += h[((int64_t)b * L + t) * C + c];
    pooled[i] = s / L;
}
__global__ void mean_pool_bwd_kernel(const float* __restrict__ dpooled, float* __restrict__ dh, int B, int L, int C) {
    const int64_t total = (int64_t)B * L * C;
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const int b = (int)(i / ((int64_t)L * C));
    dh[i] = dpooled[b * C + c] / L;
}

// logits[b][c] = pooled[b] . Wc[c] + bc[c]   (one wave per output);  dpooled[b][d] = sum_c dlogits[b][c] Wc[c][d]
__global__ void cls_fwd_kernel(const float* __restrict__ pooled, const float* __restrict__ Wc, const float* __restrict__ bc,
                               float* __restrict__ logits, int B, int C, int D) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= B * C) return;
    const int b = o / C, c = o - b * C;
    float a = 0.f;
    for (int d = lane; d < D; d += 64) a = fmaf(pooled[(int64_t)b * D + d], Wc[(int64_t)c * D + d], a);
    a = wave_sum(a);
    if (lane == 0) logits[o] = a + bc[c];
}
__global__ void cls_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ Wc, float* __restrict__ dpooled, int B,
                               int C, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * D) return;
    const int b = i / D, d = i - b * D;
    float a = 0.f;
    for (int c = 0; c < C; ++c) a = fmaf(dlogits[(int64_t)b * C + c], Wc[(int64_t)c * D + d], a);
    dpooled[i] = a;
}

// ===============================================================================================================
// 16-bit path (round 3): h16 operands, fp32 accumulation, fp32 residual stream -- the conventions of the ViT fp16 path.
// Windowed attention on the 16x16x32 h16 MFMA, one wave per (image, window, head): 49 tokens padded to 64 (4 tiles of 16),
// head_dim 32 = ONE k-step.  D[m][n]: lane (n = lane & 15, g = lane >> 4) holds rows m = 4g + i; an operand fragment is 8
// k-values per lane.  Score tiles are computed transposed (S^T[key][q]: keys on the rows), so that a lane owns one query:
// softmax statistics are per lane (+ two shuffles over g), and two stacked tiles (keys 32a + {4g.., 16 + 4g..}) ARE the B
// operand of the next product once packed to h16.  Operands whose k index is a token are read with the hardware
// transpose read in the same k order ({4g.., 16 + 4g..}).
// Per wave in LDS: Q, K, V (dO) row-major [64][32] h16, backward also P and dS as [q][key] images.
// ===============================================================================================================

constexpr int W16T = 64;                 // padded tokens of a window
// LDS layouts (bank-conflict free for every access kind below):
//   operand tiles [64 tokens][32 features] h16, 64-byte rows: 16-byte chunk c of row r stored at chunk c ^ ((r >> 2) & 3)
//   P / dS images [64 queries][64 keys] h16, 128-byte rows:   8-byte chunk c of row r stored at chunk c ^ (r & 15)
__device__ __forceinline__ int wtile_off(int r, int col) { return r * HDIM + ((((col >> 3) ^ ((r >> 2) & 3)) << 3) | (col & 7)); }
__device__ __forceinline__ int wimg_off(int r, int col) { return r * 64 + ((((col >> 2) ^ (r & 15)) << 2) | (col & 3)); }
// row fragment: lane (r, g) = X[r0 + r][8g .. 8g+7]  (k = feature)
__device__ __forceinline__ sh16x8 wfrag_row(const h16* X, int r0, int lane) {
    return *(const sh16x8*)(X + wtile_off(r0 + (lane & 15), 8 * (lane >> 4)));
}
// token-k fragment of an operand tile: lane (c, g) = { X[t0 + 4g + j][c0 + c] (j < 4), X[t0 + 16 + 4g + j - 4][c0 + c] }
__device__ __forceinline__ sh16x8 wfrag_tok_tile(const h16* X, int t0, int c0, int lane) {
    const int g4 = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const int r = t0 + 4 * g4 + q;
    return cat4(lds_read_tr16(X + wtile_off(r, c0 + 4 * p)), lds_read_tr16(X + wtile_off(r + 16, c0 + 4 * p)));
}
// the same of a P / dS image
__device__ __forceinline__ sh16x8 wfrag_tok_img(const h16* X, int t0, int c0, int lane) {
    const int g4 = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const int r = t0 + 4 * g4 + q;
    return cat4(lds_read_tr16(X + wimg_off(r, c0 + 4 * p)), lds_read_tr16(X + wimg_off(r + 16, c0 + 4 * p)));
}
__device__ __forceinline__ f32x4 wmfma(sh16x8 a, sh16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float wgmax(float v) { v = fmaxf(v, __shfl_xor(v, 16, 64)); return fmaxf(v, __shfl_xor(v, 32, 64)); }
__device__ __forceinline__ float wgsum(float v) { v += __shfl_xor(v, 16, 64); return v + __shfl_xor(v, 32, 64); }

// ---- persistent form (round 3, second version) ----------------------------------------------------------------------------
// A wave walks items gw, gw + Wn, ... (item = ((b * nW + w) * heads + hd), Wn a multiple of `heads`, so its head never
// changes).  Everything that depends on the lane and the head only is computed ONCE per kernel and kept in registers: the
// relative-position bias of each of the lane's 4 x 13 live score elements (pre-multiplied by log2 e: the softmax runs in
// base 2, `v_exp_f32` is exp2), the shift-mask bit sets, the window coordinates of the lane's tokens.  The NEXT item's
// operand rows are requested into registers before the current item is computed, so their latency hides under it.  (The
// first version -- one item per wave -- spent 25 us per item waiting: a table gather and two integer divisions per score
// element, every global load exposed at 1.25 waves per SIMD.)  Of the 64 padded keys only 49 exist: key tile 3 holds key 48
// alone (lane group g = 0, element 0); its other 15 elements are never computed.
constexpr float W16_LOG2E = 1.4426950408889634f;
constexpr int W16_NB = 13;                   // live score elements per lane and query tile: (kt, i) for kt < 3, and (3, 0)
struct WinLane {
    float bias[4][W16_NB];   // table[(qy - ky + 6) * 13 + (qx - kx + 6)][hd] * log2(e) for query tile qt, element j
    unsigned kyb, kxb;       // bit kt * 4 + i: ky >= 7 - shift, kx >= 7 - shift (region boundary inside the last window row / column)
    unsigned qyb, qxb;       // bit qt: the same of the query
    int tyx[4];              // (ty << 8) | tx of token t * 16 + n (clamped to 48): V / LSE rows, dQ / dK / dV / ctx rows
    int lyx;                 // the same of token `lane` (the operand row this lane stages)
};
__device__ __forceinline__ WinLane win_lane(int lane, int shift, const float* __restrict__ table, int heads, int hd) {
    WinLane L;
    const int n = lane & 15, g = lane >> 4, th = WS - shift;
    L.kyb = L.kxb = L.qyb = L.qxb = 0u;
    int ky[16], kx[16];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = kt * 16 + 4 * g + i, kp = key < WT ? key : WT - 1;
            ky[kt * 4 + i] = kp / WS; kx[kt * 4 + i] = kp - ky[kt * 4 + i] * WS;
            if (ky[kt * 4 + i] >= th) L.kyb |= 1u << (kt * 4 + i);
            if (kx[kt * 4 + i] >= th) L.kxb |= 1u << (kt * 4 + i);
        }
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
        const int q = qt * 16 + n, qp = q < WT ? q : WT - 1, qy = qp / WS, qx = qp - qy * WS;
        if (qy >= th) L.qyb |= 1u << qt;
        if (qx >= th) L.qxb |= 1u << qt;
        L.tyx[qt] = (qy << 8) | qx;
#pragma unroll
        for (int j = 0; j < W16_NB; ++j)
            L.bias[qt][j] = table[((qy - ky[j] + WS - 1) * (2 * WS - 1) + (qx - kx[j] + WS - 1)) * heads + hd] * W16_LOG2E;
    }
    const int lp = lane < WT ? lane : WT - 1;
    L.lyx = ((lp / WS) << 8) | (lp % WS);
    return L;
}
// keys (bit kt * 4 + i) that the shifted-window mask separates from query tile qt's query of this lane
__device__ __forceinline__ unsigned win_mask_bits(const WinLane& L, int qt, bool edge_y, bool edge_x) {
    unsigned m = 0u;
    if (edge_y) m |= ((L.qyb >> qt) & 1u) ? ~L.kyb : L.kyb;
    if (edge_x) m |= ((L.qxb >> qt) & 1u) ? ~L.kxb : L.kxb;
    return m & 0xffffu;
}
// activation row of the window token whose in-window coordinates are packed in yx; (y0, x0) = window origin + shift
__device__ __forceinline__ int64_t win_row_yx(int b, int y0, int x0, int yx, int H, int W) {
    int y = y0 + (yx >> 8), x = x0 + (yx & 0xff);
    if (y >= H) y -= H;
    if (x >= W) x -= W;
    return ((int64_t)b * H + y) * W + x;
}
// rows of one operand of the window as the lane will put them into an LDS tile: lane p < 49 holds its row's 32 features
__device__ __forceinline__ void wrow_load(sh16x8 (&v)[4], const h16* src, int64_t row, int ld, int col0, bool live) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < 8; ++k) v[c][k] = (h16)0.f;
    if (live) {
        const h16* r = src + row * ld + col0;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = *(const sh16x8*)(r + 8 * c);
    }
}
__device__ __forceinline__ void wrow_store(h16* X, const sh16x8 (&v)[4], int p) {
#pragma unroll
    for (int c = 0; c < 4; ++c) *(sh16x8*)(X + wtile_off(p, 8 * c)) = v[c];
}
// item -> image, window origin (+ shift), edge flags
struct WinItem { int b, y0, x0; bool edge_y, edge_x; };
__device__ __forceinline__ WinItem win_item(int64_t item, int heads, int nW, int nwx, int nwy, int shift) {
    const int64_t bw = item / heads;
    WinItem it;
    it.b = (int)(bw / nW);
    const int w = (int)(bw - (int64_t)it.b * nW), wy = w / nwx, wx = w - wy * nwx;
    it.y0 = wy * WS + shift; it.x0 = wx * WS + shift;
    it.edge_y = shift && wy == nwy - 1; it.edge_x = shift && wx == nwx - 1;
    return it;
}
__device__ __forceinline__ float wexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// LSE is kept in BASE 2 (log2 of the row sum of 2^(a log2 e)): the backward consumes it as it is
__global__ __launch_bounds__(64) void win16_fwd_kernel(const h16* __restrict__ qkv, int ldq, const float* __restrict__ table,
                                                       h16* __restrict__ ctx, int ldc, float* __restrict__ lse, int B, int H,
                                                       int W, int C, int heads, int shift, int64_t items) {
    __shared__ __attribute__((aligned(16))) h16 sm[3 * W16T * HDIM];
    const int lane = threadIdx.x;
    const int nwx = W / WS, nwy = H / WS, nW = nwy * nwx;
    const int64_t Wn = gridDim.x;
    const int hd = (int)(blockIdx.x % heads);
    h16 *sQ = sm, *sK = sm + W16T * HDIM, *sV = sK + W16T * HDIM;
    const WinLane L = win_lane(lane, shift, table, heads, hd);
    const int n = lane & 15, g = lane >> 4;
    const float scale2 = 0.17677669529663687f * W16_LOG2E;
    const bool live = lane < WT;
    sh16x8 pq[4], pk[4], pv[4];
    int64_t item = blockIdx.x;
    WinItem it = win_item(item, heads, nW, nwx, nwy, shift);
    auto request = [&]() {
        const int64_t row = win_row_yx(it.b, it.y0, it.x0, L.lyx, H, W);
        wrow_load(pq, qkv, row, ldq, hd * HDIM, live);
        wrow_load(pk, qkv, row, ldq, C + hd * HDIM, live);
        wrow_load(pv, qkv, row, ldq, 2 * C + hd * HDIM, live);
    };
    request();
#pragma unroll 1
    for (; item < items; item += Wn) {
        wrow_store(sQ, pq, lane);
        wrow_store(sK, pk, lane);
        wrow_store(sV, pv, lane);
        const WinItem cur = it;
        if (item + Wn < items) {                                    // next item's rows: in flight under this item's work
            it = win_item(item + Wn, heads, nW, nwx, nwy, shift);
            request();
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        auto body = [&](auto edge_c) {
            constexpr bool EDGE = decltype(edge_c)::value;
#pragma unroll
            for (int qt = 0; qt < 4; ++qt) {
                const int q = qt * 16 + n;
                const unsigned mbits = EDGE ? win_mask_bits(L, qt, cur.edge_y, cur.edge_x) : 0u;
                const sh16x8 qf = wfrag_row(sQ, qt * 16, lane);
                f32x4 st[4];
                float mx = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    st[kt] = wmfma(wfrag_row(sK, kt * 16, lane), qf, f32x4{0.f, 0.f, 0.f, 0.f});        // S^T[key][q]
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (kt == 3 && i > 0) { st[kt][i] = -INFINITY; continue; }                       // keys 49..63 do not exist
                        const int j = kt * 4 + i;
                        float a = fmaf(st[kt][i], scale2, L.bias[qt][j]);
                        if (EDGE && ((mbits >> j) & 1u)) a += -100.0f * W16_LOG2E;
                        if (kt == 3 && g != 0) a = -INFINITY;                                            // key 48 + 4g
                        st[kt][i] = a;
                        mx = fmaxf(mx, a);
                    }
                }
                mx = wgmax(mx);
                float sum = 0.f;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (kt == 3 && i > 0) { st[kt][i] = 0.f; continue; }
                        st[kt][i] = wexp2(st[kt][i] - mx);
                        sum += st[kt][i];
                    }
                sum = wgsum(sum);
                f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    sh16x8 pb;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { pb[j] = f2h(st[2 * a][j]); pb[4 + j] = f2h(st[2 * a + 1][j]); }
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) o[dt] = wmfma(wfrag_tok_tile(sV, 32 * a, dt * 16, lane), pb, o[dt]);   // O^T[d][q]
                }
                if (q < WT) {
                    const float inv = 1.f / sum;
                    const int64_t row = win_row_yx(cur.b, cur.y0, cur.x0, L.tyx[qt], H, W);
                    h16* dst = ctx + row * ldc + hd * HDIM;
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        sh16x4 ov;
#pragma unroll
                        for (int i = 0; i < 4; ++i) ov[i] = f2h(o[dt][i] * inv);
                        *(sh16x4*)(dst + dt * 16 + 4 * g) = ov;
                    }
                    if (g == 0) lse[row * heads + hd] = mx + __log2f(sum);
                }
            }
        };
        if (cur.edge_y || cur.edge_x) body(std::true_type{}); else body(std::false_type{});
    }
}

constexpr int PLD = 64;                  // row stride of the P / dS images ([q][key] h16)
// LDS per wave: Q, K, dO tiles (V is only ever read as row fragments: straight from global memory) + the P and dS images
// = 28 KiB; the kernel runs one wave per SIMD (its registers: 64 of prefetch, 52 of bias), four workgroups per CU
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void win16_bwd_kernel(const h16* __restrict__ qkv, int ldq, const float* __restrict__ table,
                                                       const h16* __restrict__ dctx, int ldc, const float* __restrict__ lse,
                                                       h16* __restrict__ dqkv, int B, int H, int W, int C, int heads,
                                                       int shift, int64_t items) {
    __shared__ __attribute__((aligned(16))) h16 sm[3 * W16T * HDIM + 2 * W16T * PLD];
    const int lane = threadIdx.x;
    const int nwx = W / WS, nwy = H / WS, nW = nwy * nwx;
    const int64_t Wn = gridDim.x;
    const int hd = (int)(blockIdx.x % heads);
    h16 *sQ = sm, *sK = sQ + W16T * HDIM, *sdO = sK + W16T * HDIM, *sP = sdO + W16T * HDIM, *sdS = sP + W16T * PLD;
    const WinLane L = win_lane(lane, shift, table, heads, hd);
    const int n = lane & 15, g = lane >> 4;
    const float scale = 0.17677669529663687f, scale2 = scale * W16_LOG2E;
    const bool live = lane < WT;
    sh16x8 pq[4], pk[4], pd[4], pvf[4];
    float plse[4];
    int64_t prow[4];
    int64_t item = blockIdx.x;
    WinItem it = win_item(item, heads, nW, nwx, nwy, shift);
    auto request = [&]() {
        const int64_t row = win_row_yx(it.b, it.y0, it.x0, L.lyx, H, W);
        wrow_load(pq, qkv, row, ldq, hd * HDIM, live);
        wrow_load(pk, qkv, row, ldq, C + hd * HDIM, live);
        wrow_load(pd, dctx, row, ldc, hd * HDIM, live);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool lv = t * 16 + n < WT;                            // V row fragment of key tile t / LSE of query tile t
            prow[t] = win_row_yx(it.b, it.y0, it.x0, L.tyx[t], H, W);   // (clamped token: always a valid row)
#pragma unroll
            for (int k = 0; k < 8; ++k) pvf[t][k] = (h16)0.f;
            if (lv) pvf[t] = *(const sh16x8*)(qkv + prow[t] * ldq + 2 * C + hd * HDIM + 8 * g);
            plse[t] = lv ? lse[prow[t] * heads + hd] : INFINITY;        // rows >= 49: P = 0
        }
    };
    request();
#pragma unroll 1
    for (; item < items; item += Wn) {
        wrow_store(sQ, pq, lane);
        wrow_store(sK, pk, lane);
        wrow_store(sdO, pd, lane);
        // REAL copies (v_mov the compiler cannot fold away): the item works on registers that are not load destinations, so
        // every wait on the previous request sits here, before the next one is issued -- vmcnt is in order, and a wait for
        // an old load inside the item's work would also wait for the first of the new ones
        sh16x8 vf[4];
        float lq[4];
        int64_t crow[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            const u32x4 src = __builtin_bit_cast(u32x4, pvf[t]);
            u32x4 dstv;
#pragma unroll
            for (int k = 0; k < 4; ++k) { unsigned o; asm volatile("v_mov_b32 %0, %1" : "=v"(o) : "v"(src[k])); dstv[k] = o; }
            vf[t] = __builtin_bit_cast(sh16x8, dstv);
            asm volatile("v_mov_b32 %0, %1" : "=v"(lq[t]) : "v"(plse[t]));
            crow[t] = prow[t];
        }
        const WinItem cur = it;
        if (item + Wn < items) {
            it = win_item(item + Wn, heads, nW, nwx, nwy, shift);
            request();
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // ---- per query tile: P^T, dS^T (keys on the rows); dQ from them directly, P / dS also into the [q][key] images ----
        auto body = [&](auto edge_c) {
            constexpr bool EDGE = decltype(edge_c)::value;
#pragma unroll
            for (int qt = 0; qt < 4; ++qt) {
                const int q = qt * 16 + n;
                const unsigned mbits = EDGE ? win_mask_bits(L, qt, cur.edge_y, cur.edge_x) : 0u;
                const sh16x8 qf = wfrag_row(sQ, qt * 16, lane), dof = wfrag_row(sdO, qt * 16, lane);
                f32x4 p[4], dp[4];
                float dsum = 0.f;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    p[kt] = wmfma(wfrag_row(sK, kt * 16, lane), qf, f32x4{0.f, 0.f, 0.f, 0.f});          // S^T[key][q]
                    dp[kt] = wmfma(vf[kt], dof, f32x4{0.f, 0.f, 0.f, 0.f});                              // dP^T[key][q]
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (kt == 3 && i > 0) { p[kt][i] = 0.f; dp[kt][i] = 0.f; continue; }              // keys 49..63 do not exist
                        const int j = kt * 4 + i;
                        float a = fmaf(p[kt][i], scale2, L.bias[qt][j]);
                        if (EDGE && ((mbits >> j) & 1u)) a += -100.0f * W16_LOG2E;
                        float pv = wexp2(a - lq[qt]);
                        if (kt == 3 && g != 0) pv = 0.f;                                                  // key 48 + 4g
                        p[kt][i] = pv;
                        dsum = fmaf(pv, dp[kt][i], dsum);
                    }
                }
                const float delta = wgsum(dsum);                 // rowsum(P * dP) = rowsum(dO * O)
                f32x4 dq[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    sh16x4 p4, d4;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (kt == 3 && i > 0) { p4[i] = (h16)0.f; d4[i] = (h16)0.f; continue; }
                        dp[kt][i] = p[kt][i] * (dp[kt][i] - delta) * scale;        // dS^T
                        p4[i] = f2h(p[kt][i]);
                        d4[i] = f2h_sat(dp[kt][i]);
                    }
                    // images [q][key]: this lane's query row, keys 16kt + 4g .. +3
                    *(sh16x4*)(sP + wimg_off(q, kt * 16 + 4 * g)) = p4;
                    *(sh16x4*)(sdS + wimg_off(q, kt * 16 + 4 * g)) = d4;
                }
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    sh16x8 db;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { db[j] = f2h_sat(dp[2 * a][j]); db[4 + j] = f2h_sat(dp[2 * a + 1][j]); }
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) dq[dt] = wmfma(wfrag_tok_tile(sK, 32 * a, dt * 16, lane), db, dq[dt]);   // dQ^T[d][q]
                }
                if (q < WT) {
                    h16* dst = dqkv + crow[qt] * ldq + hd * HDIM;
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        sh16x4 ov;
#pragma unroll
                        for (int i = 0; i < 4; ++i) ov[i] = f2h_sat(dq[dt][i]);
                        *(sh16x4*)(dst + dt * 16 + 4 * g) = ov;
                    }
                }
            }
        };
        if (cur.edge_y || cur.edge_x) body(std::true_type{}); else body(std::false_type{});
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // ---- per key tile: dV^T[d][key] = sum_q dO^T[d][q] P[q][key], dK^T[d][key] = sum_q Q^T[d][q] dS[q][key] ----
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const int key = kt * 16 + n;
            f32x4 dv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, dk[2] = {dv[0], dv[0]};
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const sh16x8 pb = wfrag_tok_img(sP, 32 * a, kt * 16, lane), db = wfrag_tok_img(sdS, 32 * a, kt * 16, lane);   // k = query, n = key
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    dv[dt] = wmfma(wfrag_tok_tile(sdO, 32 * a, dt * 16, lane), pb, dv[dt]);
                    dk[dt] = wmfma(wfrag_tok_tile(sQ, 32 * a, dt * 16, lane), db, dk[dt]);
                }
            }
            if (key < WT) {
                h16* dst = dqkv + crow[kt] * ldq + hd * HDIM;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    sh16x4 kv, vv;
#pragma unroll
                    for (int i = 0; i < 4; ++i) { kv[i] = f2h_sat(dk[dt][i]); vv[i] = f2h_sat(dv[dt][i]); }
                    *(sh16x4*)(dst + C + dt * 16 + 4 * g) = kv;
                    *(sh16x4*)(dst + 2 * C + dt * 16 + 4 * g) = vv;
                }
            }
        }
        // the next item's LDS writes follow this item's last LDS reads in program order of the one wave: no barrier needed
    }
}

// persistent grid of the window kernels: `per_cu` single-wave workgroups per CU, a multiple of `heads`, at most one per item
int g_win_bwd_per_cu = 5;    // VITLORA_SWIN_WIN_BWD: single-wave workgroups of the backward window kernel per CU (LDS: 28 KB each -> 5; registers: 2 per SIMD since round 5)
int g_win_cus = 256;       // VITLORA_SWIN_WIN_CUS: CUs a window-attention launch is sized for (A/B knob: half the chip per chain when two chains run)
inline unsigned win16_grid(int64_t items, int heads, int per_cu) {
    int64_t wn = (int64_t)g_win_cus * per_cu / heads * heads;
    if (wn > items) wn = items;          // items is a multiple of heads
    return (unsigned)wn;
}

// out[b][i] = x[b][i] * f[b]  (per-image power-of-two gradient scale of the 16-bit backward and its inverse)
__global__ void scale_rows_kernel(const float* __restrict__ x, const float* __restrict__ f, float* __restrict__ out, int B, int64_t n) {
    const int64_t total = (int64_t)B * n, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += stride) out[i] = x[i] * f[i / n];
}

inline unsigned nblk(int64_t n, int t, int cap) {
    int64_t b = (n + t - 1) / t;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

struct SLora { int row_off, out; float *A, *B; };            // one adapted module inside a (fused) linear
struct SLin {
    int out = 0, in = 0;
    float *W = nullptr, *b = nullptr;
    std::vector<SLora> slots;
    // 16-bit path: operands zero-padded to multiples of 128 in both directions (the h16 GEMM kernels' tile sizes)
    int inP = 0, outP = 0, kext = 0;          // widths in the K role (multiples of 128)
    int inN = 0, outN = 0;                    // widths in the N role (round 5): a multiple of 256 where that puts the GEMM on the 256-wide
                                              // tile kernels (C = 384: N = 384 -> 512, 1152 -> 1280; the extra weight rows are zero)
    h16 *W16 = nullptr, *WT16 = nullptr;      // [outN][inP], [inN][outP]
    float* b16 = nullptr;                     // [outN] fp32, zero padded
    h16 *Ad = nullptr, *Bu = nullptr, *Bd = nullptr, *Au = nullptr;   // [64][inP], [outN][64] (scaled), [64][outP], [inN][64] (scaled)
};
// What is fixed at vl_swin_create / swin16_commit: weights, packed operands, LoRA slots and the 16-bit path's layout of a stage.
struct SBlock {
    SLin qkv, o, fc1, fc2;
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *table;
};
struct SStage {
    int C, H, heads, depth;
    std::vector<SBlock> blocks;
    // downsample (absent after the last stage)
    float *mg_g = nullptr, *mg_b = nullptr, *Wred = nullptr;
    h16 *Wred16 = nullptr, *WredT16 = nullptr;      // patch-merging reduction on h16 operands
    // 16-bit path: layout of the stage's activations (strides are the stage's own padded widths: pad columns stay zero for ever)
    int CP = 0, C3P = 0, C4P = 0;             // GEMM dims: C, 3C, 4C rounded up to the 128-wide tiles (weights are zero padded)
    int LD = 0;                               // row stride of the GEMM RESULTS of width C (delta16, dh16, dctx16): LC, or the N-role width of C
    int LC = 0, L3 = 0, L4 = 0;               // row strides of the h16 activations: the padded dims, or C, 3C, 4C themselves
                                              // (stage 1: 96 / 288 / 384 -- a quarter fewer bytes on every tensor of the HBM-bound
                                              // stage; the GEMM then reads its last K columns from the NEXT row, times zero weights,
                                              // and skips the stores of the tile grid's extra columns: GemmArgs.n_store)
};

// What swin_carve lays out: the activations of ONE forward / backward chain and what its last forward left behind.  The handle owns
// one for the whole batch and one per chain of vl_swin_pgd_attack; the launch sequences take the one they work on as an argument.
struct SBlockWs {       // saved by the forward
    float *xa, *xb, *mean1, *rstd1, *mean2, *rstd2, *qkvbuf, *ctx, *lse, *z;
    h16 *qkv16 = nullptr, *z16 = nullptr;     // 16-bit path: [Rp][P(3C)], gelu'(z) [Rp][P(4C)]
    h16 *xa16 = nullptr, *xb16 = nullptr;     // 16-bit path (round 5): the residual stream entering LayerNorm 1 / LayerNorm 2, h16 [Rp][C]
};
struct SStageWs {
    std::vector<SBlockWs> blocks;
    float *mg = nullptr, *mmean = nullptr, *mrstd = nullptr;    // patch merging, saved
    // 16-bit path: per-stage scratch
    h16 *h16b = nullptr, *a16 = nullptr, *delta16 = nullptr, *ctx16 = nullptr, *t16 = nullptr, *u16 = nullptr;
    h16 *dz16 = nullptr, *dqkv16 = nullptr, *dh16 = nullptr, *dctx16 = nullptr, *gh16 = nullptr;
    h16 *mg16 = nullptr, *g16 = nullptr;
};
struct SwinWs {
    int max_batch = 0, cur_B = 0, cur_norm = 0, have_loss = 0;     // (main workspace: max_batch < 0 = planned for -max_batch, not armed)
    SStageWs st[4];
    float *patches, *emb, *emean, *erstd, *xlast, *fmean, *frstd, *hfin, *pooled, *logits, *dlogits, *loss, *loss_img, *dpooled;
    float *h, *a, *t, *u, *g0, *g1, *dbig, *dqkv, *grad_img, *stage_x0, *stage_adv;
    int64_t* stage_labels;
    float *gscale = nullptr, *inv_gscale = nullptr, *dlogits_s = nullptr;
    h16 *patches16 = nullptr, *emb16 = nullptr;    // [R0][48], [R0][E]
    h16 *xlast16 = nullptr, *hfin16 = nullptr, *dhfin16 = nullptr;      // 16-bit path: last stage's output stream, final LayerNorm output, its gradient
};

}  // namespace
}  // namespace VLNS (reopened below: the handle is the global type include/vitlora.h declares)
using namespace VLNS;

struct vl_swin {
    vl_swin_config cfg;
    int S, P, G0, E, C, r;
    float scaling;
    std::vector<SStage> stages;
    float *Wpe, *bpe, *eg, *eb, *fg, *fb, *Wc, *bc;
    float* flat = nullptr;
    int64_t flat_n = 0;
    std::vector<void*> allocs;
    SwinWs w;                // the whole-batch workspace
    int* err_flag = nullptr;
    float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    h16 *Wpe16 = nullptr, *WpeT16 = nullptr;      // 16-bit patch embedding (P = 4): [128][64] (rows >= E, columns >= 48 zero), [128][128] (rows >= 48 zero)
    float* bpe16 = nullptr;                        // [128] fp32, zero padded
    int pe16 = 0;                                  // the 16-bit patch embedding is in use (P == 4, E <= 128; VITLORA_SWIN_PE16=0: fp32 form of rounds 3-4)
    int f16 = 0;             // cfg.reserved[0] == 1: 16-bit operand path for the blocks (embedding, merging and head stay fp32)
    int dirty = 1;           // packed h16 operands are stale (weights / adapters written since the last commit)
    // vl_swin_pgd_attack as TWO half-batch chains on two streams (round 5; the ViT path got them in round 4): stages 3-4 are
    // small-batch shaped at any batch (M = 50 176 / 12 544 rows: 392 / 147 tiles on 256 CUs) and the window kernels run one or two waves
    // per SIMD, so the ends of one chain's kernels meet the main loops of the other's.  Each chain is a workspace of its own, driven
    // with this same handle; they are carved into the SAME planned bytes as the main workspace (never live together).
    static constexpr int MAXCH = 4;
    SwinWs chain[MAXCH];
    int chain_batch = 0, chains_on = 2, chain_min = 32;      // VITLORA_SWIN_CHAINS = number of chains (0 / 1: off, default 2, at most 4); VITLORA_SWIN_CHAIN_MIN: smallest batch that is split
    hipStream_t side[MAXCH - 1] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int unpad_stages = 3;    // bit i: stage i keeps its h16 activations at their true width (VITLORA_SWIN_UNPAD; default since round 5: stages 1 and 2, C = 96 / 192 -- every h16 activation is then dense, there are no pad columns at all; stage 2 alone is time-neutral)
};

namespace VLNS {

namespace {

template <typename Tp>
int salloc(vl_swin* m, Tp** p, size_t n) {
    void* q = nullptr;
    if (hipMalloc(&q, n * sizeof(Tp) + 256) != hipSuccess) return vl_fail(VL_ERR_HIP, "hipMalloc(%zu) failed", n * sizeof(Tp));
    if (hipMemset(q, 0, n * sizeof(Tp) + 256) != hipSuccess) return vl_fail(VL_ERR_HIP, "hipMemset failed");
    m->allocs.push_back(q);
    *p = (Tp*)q;
    return VL_OK;
}

GemmF32 gm(const float* A, int lda, const float* W, int ldw, int transW, int M, int N, int K, float* C, int ldc) {
    GemmF32 g;
    memset(&g, 0, sizeof g);
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.transW = transW;
    g.M = M; g.Mstore = M; g.N = N; g.K = K; g.alpha = 1.f; g.C = C; g.ldc = ldc;
    return g;
}

// y = x W^T + b (+ R) + sum over adapted modules of s * (x A^T) B^T        (peft lora.Linear, eval mode)
void lin_fwd(const vl_swin* m, SwinWs& w, const SLin& ln, const float* x, int M, float* y, const float* R, hipStream_t s) {
    GemmF32 g = gm(x, ln.in, ln.W, ln.in, 0, M, ln.out, ln.in, y, ln.out);
    g.bias = ln.b; g.R = R; g.ldr = ln.out;
    k_gemm_f32(g, s);
    for (const SLora& sl : ln.slots) {
        k_gemm_f32(gm(x, ln.in, sl.A, ln.in, 0, M, m->r, ln.in, w.t, 64), s);
        GemmF32 u = gm(w.t, 64, sl.B, m->r, 0, M, sl.out, m->r, y + sl.row_off, ln.out);
        u.alpha = m->scaling; u.R = y + sl.row_off; u.ldr = ln.out;
        k_gemm_f32(u, s);
    }
}
// dx = dy W + sum of s * (dy B) A
void lin_dgrad(const vl_swin* m, SwinWs& w, const SLin& ln, const float* dy, int M, float* dx, hipStream_t s) {
    k_gemm_f32(gm(dy, ln.out, ln.W, ln.in, 1, M, ln.in, ln.out, dx, ln.in), s);
    for (const SLora& sl : ln.slots) {
        k_gemm_f32(gm(dy + sl.row_off, ln.out, sl.B, m->r, 1, M, m->r, sl.out, w.u, 64), s);
        GemmF32 a = gm(w.u, 64, sl.A, ln.in, 1, M, ln.in, m->r, dx, ln.in);
        a.alpha = m->scaling; a.R = dx; a.ldr = ln.in;
        k_gemm_f32(a, s);
    }
}

// ---- 16-bit path: packed operands, block forward / backward --------------------------------------------------------------
inline int padc(int c) { return (int)round_up(c, 128); }
// N-role width of a padded dimension `n` in a stage of width C: stages whose token count puts their GEMMs on the 256-wide tile
// kernels (C >= 384: M <= 50 176 rows at batch 256) round N up to a multiple of 256 -- 128-column remainders (384, 1152) otherwise
// send the whole product to the 128 x 128 kernel at half the rate (round 5: 2.5 ms of a 20.6 ms step)
inline int npad(int C, int n) { return (C >= 384 && n % 256) ? (int)round_up(n, 256) : n; }

GemmArgs ga(const h16* A, int lda, const h16* W, int ldw, int K, int M, int N) {
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A1 = A; g.lda1 = lda; g.W1 = W; g.ldw1 = ldw; g.K1 = K; g.M = M; g.Mvalid = M; g.N = N;
    return g;
}

// first LoRA column of a slot inside the 64-wide K extension (q, k, v of the fused projection at 0, r, 2r)
inline int ext_off_of(const vl_swin* m, const SLin& ln, const SLora& sl) { return ln.slots.size() == 3 ? (sl.row_off / (ln.out / 3)) * m->r : 0; }

// re-derive every h16 operand from the fp32 masters (weights, biases, adapters); idempotent
void swin16_commit(vl_swin* m, hipStream_t s) {
    for (SStage& st : m->stages)
        for (SBlock& bk : st.blocks)
            for (SLin* ln : {&bk.qkv, &bk.o, &bk.fc1, &bk.fc2}) {
                k_pack_h16(ln->W, ln->W16, ln->out, ln->in, ln->inP, 0, 1.f, s);
                k_pack_h16_t(ln->W, ln->WT16, ln->out, ln->in, ln->outP, 0, 1.f, s);
                (void)hipMemcpyAsync(ln->b16, ln->b, (size_t)ln->out * sizeof(float), hipMemcpyDeviceToDevice, s);
                for (const SLora& sl : ln->slots) {
                    const int eo = ext_off_of(m, *ln, sl);
                    k_pack_h16(sl.A, ln->Ad + (size_t)eo * ln->inP, m->r, ln->in, ln->inP, 0, 1.f, s);
                    k_pack_h16(sl.B, ln->Bu + (size_t)sl.row_off * 64, sl.out, m->r, 64, eo, m->scaling, s);
                    k_pack_h16_t(sl.B, ln->Bd + (size_t)eo * ln->outP, sl.out, m->r, ln->outP, sl.row_off, 1.f, s);
                    k_pack_h16_t(sl.A, ln->Au, m->r, ln->in, 64, eo, m->scaling, s);
                }
            }
    if (m->pe16) {
        const int PK = 3 * m->P * m->P;
        k_pack_h16(m->Wpe, m->Wpe16, m->E, PK, 64, 0, 1.f, s);
        k_pack_h16_t(m->Wpe, m->WpeT16, m->E, PK, 128, 0, 1.f, s);
        (void)hipMemcpyAsync(m->bpe16, m->bpe, (size_t)m->E * sizeof(float), hipMemcpyDeviceToDevice, s);
    }
    for (int i = 0; i < 3; ++i) {
        SStage& st = m->stages[i];
        k_pack_h16(st.Wred, st.Wred16, 2 * st.C, 4 * st.C, 4 * st.C, 0, 1.f, s);
        k_pack_h16_t(st.Wred, st.WredT16, 2 * st.C, 4 * st.C, 2 * st.C, 0, 1.f, s);
    }
    m->dirty = 0;
}

// y = x W^T + b (+ LoRA as one extra K tile), epilogue `epi`; x [Mp][inP] h16
void lin16_fwd(const vl_swin* m, SStageWs& sw, const SLin& ln, const h16* x, int ldx, int Mp, int M, GemmArgs g, int epi, hipStream_t s) {
    g.A1 = x; g.lda1 = ldx; g.W1 = ln.W16; g.ldw1 = ln.inP; g.K1 = ln.inP;
    g.M = Mp; g.Mvalid = M; g.N = ln.outN; g.bias = ln.b16; g.no_pp = 1;
    g.n_store = g.ldc < ln.outN ? ln.out : 0;                      // unpadded result rows (ldc = out)
    if (ln.kext) {
        g.W2 = ln.Bu; g.ldw2 = 64; g.K2 = 64;
        g.k2_algo = m->r; g.k2_used = m->r * (int)ln.slots.size();
        g.down_W = ln.Ad; g.down_ldw = ln.inP; g.down_groups = 1;
        // the down projection rides inside the GEMM where a kernel can carry it: the streaming kernel (stages 1-2)
        if (!gemm_stream_fuses_down(g, epi)) {          // t = x Ad^T as its own skinny GEMM, read back as the LoRA K tile's A operand
            g.down_W = nullptr; g.down_ldw = 0; g.down_groups = 0;
            GemmArgs d = ga(x, ldx, ln.Ad, ln.inP, ln.inP, Mp, 64);
            d.Mvalid = M; d.C = sw.t16; d.ldc = 64; d.n_algo = m->r * (int)ln.slots.size();
            launch_gemm(d, EPI_STORE_H16, 64, s);
            g.A2 = sw.t16; g.lda2 = 64;
        }
    }
    launch_gemm(g, epi, 128, s);
}
// dx = dy W (+ LoRA), dy [Mp][outP] h16
void lin16_dgrad(const vl_swin* m, SStageWs& sw, const SLin& ln, const h16* dy, int ldy, int Mp, int M, GemmArgs g, int epi, hipStream_t s) {
    g.A1 = dy; g.lda1 = ldy; g.W1 = ln.WT16; g.ldw1 = ln.outP; g.K1 = ln.outP;
    g.M = Mp; g.Mvalid = M; g.N = ln.inN; g.bias = nullptr; g.no_pp = 1;
    g.n_store = g.ldc < ln.inN ? ln.in : 0;
    if (ln.kext) {
        g.W2 = ln.Au; g.ldw2 = 64; g.K2 = 64;
        g.k2_algo = m->r * (int)ln.slots.size(); g.k2_used = g.k2_algo;
        g.down_W = ln.Bd; g.down_ldw = ln.outP; g.down_groups = 1;
        if (!gemm_stream_fuses_down(g, epi)) {
            g.down_W = nullptr; g.down_ldw = 0; g.down_groups = 0;
            GemmArgs d = ga(dy, ldy, ln.Bd, ln.outP, ln.outP, Mp, 64);
            d.Mvalid = M; d.C = sw.u16; d.ldc = 64; d.n_algo = m->r;
            launch_gemm(d, EPI_STORE_H16, 64, s);
            g.A2 = sw.u16; g.lda2 = 64;
        }
    }
    launch_gemm(g, epi, 128, s);
}

// One Swin block, forward, on the 16-bit residual stream (round 5).  x_prev16: the stream entering the PREVIOUS block's MLP
// (its xb16) when `add_delta` -- sw.delta16 then still holds that block's fc2 output and LayerNorm 1 adds the two on its way
// (x' = round16(x + delta) -> bw.xa16); otherwise bw.xa16 already is this block's input (first block of a stage).  Leaves the
// block's own fc2 output in sw.delta16 (to be added by whoever consumes the stream next) and the stream before it in bw.xb16.
void swin16_block_fwd(const vl_swin* m, const SStage& st, SStageWs& sw, const SBlock& bk, SBlockWs& bw, const h16* x_prev16, bool add_delta, int B, int shift, hipStream_t s) {
    const int Cs = st.C, Hs = st.H, M = B * Hs * Hs, Mp = (int)round_up(M, 128);
    const int nW = (Hs / WS) * (Hs / WS);
    GemmArgs g;
    if (add_delta) sw_ln_fwd16<false>(x_prev16, Cs, sw.delta16, st.LD, bw.xa16, Cs, sw.h16b, st.LC, bw.mean1, bw.rstd1, bk.ln1_g, bk.ln1_b, M, Cs, m->cfg.ln_eps, m->err_flag, s);
    else sw_ln_fwd16<false>(bw.xa16, Cs, nullptr, 0, nullptr, 0, sw.h16b, st.LC, bw.mean1, bw.rstd1, bk.ln1_g, bk.ln1_b, M, Cs, m->cfg.ln_eps, m->err_flag, s);
    memset(&g, 0, sizeof g); g.C = bw.qkv16; g.ldc = st.L3;
    lin16_fwd(m, sw, bk.qkv, sw.h16b, st.LC, Mp, M, g, EPI_STORE_H16, s);
    const int64_t witems = (int64_t)B * nW * st.heads;
    if (g_poison_lds) vl_poison_lds(s);      // test hook (prof.h): the window kernels keep K / V / Q / dO of a window in LDS
    hipLaunchKernelGGL(win16_fwd_kernel, dim3(win16_grid(witems, st.heads, 8)), dim3(64), 0, s,
                       bw.qkv16, st.L3, bk.table, sw.ctx16, st.LC, bw.lse, B, Hs, Hs, Cs, st.heads, shift, witems);
    memset(&g, 0, sizeof g); g.C = sw.delta16; g.ldc = st.LD;
    lin16_fwd(m, sw, bk.o, sw.ctx16, st.LC, Mp, M, g, EPI_STORE_H16, s);
    // LayerNorm 2 (+ residual add of the attention output: xa16 + delta -> xb16)
    sw_ln_fwd16<false>(bw.xa16, Cs, sw.delta16, st.LD, bw.xb16, Cs, sw.h16b, st.LC, bw.mean2, bw.rstd2, bk.ln2_g, bk.ln2_b, M, Cs, m->cfg.ln_eps, m->err_flag, s);
    memset(&g, 0, sizeof g); g.C = sw.a16; g.ldc = st.L4; g.C2 = bw.z16; g.ldc2 = st.L4;
    lin16_fwd(m, sw, bk.fc1, sw.h16b, st.LC, Mp, M, g, EPI_GELU, s);
    memset(&g, 0, sizeof g); g.C = sw.delta16; g.ldc = st.LD;
    lin16_fwd(m, sw, bk.fc2, sw.a16, st.L4, Mp, M, g, EPI_STORE_H16, s);
}

// One Swin block, backward.  sw.gh16 (h16, row stride st.LC) holds the gradient w.r.t. the block's output stream and is updated
// IN PLACE to the gradient w.r.t. its input stream: it is the residual-gradient stream and the A operand of the dgrad GEMMs.
void swin16_block_bwd(const vl_swin* m, const SStage& st, SStageWs& sw, const SBlock& bk, SBlockWs& bw, int B, int shift, hipStream_t s) {
    const int Cs = st.C, Hs = st.H, M = B * Hs * Hs, Mp = (int)round_up(M, 128);
    const int nW = (Hs / WS) * (Hs / WS);
    GemmArgs g;
    memset(&g, 0, sizeof g); g.C = sw.dz16; g.ldc = st.L4; g.R = bw.z16; g.ldr = st.L4;
    lin16_dgrad(m, sw, bk.fc2, sw.gh16, st.LC, Mp, M, g, EPI_GELU_BWD, s);                         // d(z) = (d(out) Wfc2) * gelu'(z)
    memset(&g, 0, sizeof g); g.C = sw.dh16; g.ldc = st.LD;
    lin16_dgrad(m, sw, bk.fc1, sw.dz16, st.L4, Mp, M, g, EPI_STORE_H16, s);
    sw_ln_bwd16<false, false>(sw.dh16, st.LD, bw.xb16, Cs, bw.mean2, bw.rstd2, bk.ln2_g, sw.gh16, sw.gh16, st.LC, M, Cs, m->err_flag, s);
    memset(&g, 0, sizeof g); g.C = sw.dctx16; g.ldc = st.LD;
    lin16_dgrad(m, sw, bk.o, sw.gh16, st.LC, Mp, M, g, EPI_STORE_H16, s);
    const int64_t witems = (int64_t)B * nW * st.heads;
    if (g_poison_lds) vl_poison_lds(s);      // test hook (prof.h): the window kernels keep K / V / Q / dO of a window in LDS
    hipLaunchKernelGGL(win16_bwd_kernel, dim3(win16_grid(witems, st.heads, g_win_bwd_per_cu)), dim3(64), 0, s,
                       bw.qkv16, st.L3, bk.table, sw.dctx16, st.LD, bw.lse, sw.dqkv16, B, Hs, Hs, Cs, st.heads, shift, witems);
    memset(&g, 0, sizeof g); g.C = sw.dh16; g.ldc = st.LD;
    lin16_dgrad(m, sw, bk.qkv, sw.dqkv16, st.L3, Mp, M, g, EPI_STORE_H16, s);
    sw_ln_bwd16<false, false>(sw.dh16, st.LD, bw.xa16, Cs, bw.mean1, bw.rstd1, bk.ln1_g, sw.gh16, sw.gh16, st.LC, M, Cs, m->err_flag, s);
}

int parse2(const char* name, const char* pfx, int* a, const char** rest) {
    const size_t n = strlen(pfx);
    if (strncmp(name, pfx, n) != 0) return 0;
    char* end = nullptr;
    long v = strtol(name + n, &end, 10);
    if (end == name + n || *end != '.') return 0;
    *a = (int)v; *rest = end + 1;
    return 1;
}

}  // namespace

extern "C" {

int vl_swin_create(const vl_swin_config* cfg, vl_swin** out) {
    if (!cfg || !out) return vl_fail(VL_ERR_ARG, "null argument");
    if (cfg->window != WS) return vl_fail(VL_ERR_UNSUPPORTED, "window must be 7");
    if (cfg->image_size % cfg->patch_size) return vl_fail(VL_ERR_UNSUPPORTED, "image_size %% patch_size != 0");
    if (cfg->lora_r < 0 || cfg->lora_r > 16 || cfg->lora_r % 4) return vl_fail(VL_ERR_UNSUPPORTED, "lora_r must be 0, 4, 8, 12 or 16");
    int res = cfg->image_size / cfg->patch_size;
    for (int i = 0; i < 4; ++i) {
        const int Cst = cfg->embed_dim << i;
        if (cfg->depths[i] <= 0 || cfg->heads[i] <= 0 || Cst != cfg->heads[i] * HDIM)
            return vl_fail(VL_ERR_UNSUPPORTED, "stage %d: head_dim must be 32 (dim %d, heads %d)", i, Cst, cfg->heads[i]);
        if (res % WS) return vl_fail(VL_ERR_UNSUPPORTED, "stage %d: resolution %d is not a multiple of the window", i, res);
        if (i < 3 && (res & 1)) return vl_fail(VL_ERR_UNSUPPORTED, "stage %d: odd resolution cannot be merged", i);
        if (4 * Cst > 2048 && i < 3) return vl_fail(VL_ERR_UNSUPPORTED, "patch-merging width exceeds the LayerNorm kernel");
        if (i < 3) res /= 2;
    }
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (int e = f32_init(dev)) return vl_fail(VL_ERR_HIP, "f32_init failed (%d)", e);
    if (cfg->reserved[0] != 0 && cfg->reserved[0] != 1) return vl_fail(VL_ERR_ARG, "precision (reserved[0]) must be 0 (f32) or 1 (f16)");
    if (cfg->reserved[0] == 1)
        if (int e = gemm_init(dev)) return vl_fail(VL_ERR_HIP, "gemm_init: hipFuncSetAttribute failed (%d)", e);
    vl_swin* m = new vl_swin();
    m->cfg = *cfg;
    m->f16 = cfg->reserved[0] == 1;
    m->unpad_stages = env_int("VITLORA_SWIN_UNPAD", m->unpad_stages);
    m->chains_on = std::min(env_int("VITLORA_SWIN_CHAINS", m->chains_on), (int)vl_swin::MAXCH);
    m->chain_min = env_int("VITLORA_SWIN_CHAIN_MIN", m->chain_min);
    g_win_cus = env_int("VITLORA_SWIN_WIN_CUS", g_win_cus);
    g_win_bwd_per_cu = env_int("VITLORA_SWIN_WIN_BWD", g_win_bwd_per_cu);
    m->S = cfg->image_size; m->P = cfg->patch_size; m->G0 = m->S / m->P; m->E = cfg->embed_dim; m->C = cfg->num_labels;
    m->r = cfg->lora_targets ? cfg->lora_r : 0;
    m->scaling = m->r ? cfg->lora_alpha / (float)m->r : 0.f;
    int rc;
#define A_(p, n) if ((rc = salloc(m, &(p), (size_t)(n))) != VL_OK) { vl_swin_destroy(m); return rc; }
    const int PK = 3 * m->P * m->P;
    A_(m->Wpe, (size_t)m->E * PK); A_(m->bpe, m->E); A_(m->eg, m->E); A_(m->eb, m->E);
    m->pe16 = m->f16 && m->P == 4 && m->E <= 128 && m->E % 32 == 0;
    m->pe16 = m->pe16 && env_int("VITLORA_SWIN_PE16", 1) != 0;
    if (m->pe16) { A_(m->Wpe16, (size_t)128 * 64); A_(m->WpeT16, (size_t)128 * 128); A_(m->bpe16, 128); }
    // flat LoRA buffer layout: [stage][block][target q,k,v,o,fc1,fc2]{A, B}
    int64_t off = 0;
    m->stages.resize(4);
    res = m->G0;
    for (int i = 0; i < 4; ++i) {
        SStage& st = m->stages[i];
        st.C = m->E << i; st.H = res; st.heads = cfg->heads[i]; st.depth = cfg->depths[i];
        st.blocks.resize(st.depth);
        const int Cs = st.C;
        if (m->f16) {
            st.CP = padc(Cs); st.C3P = padc(3 * Cs); st.C4P = padc(4 * Cs);
            const bool unpad = ((m->unpad_stages >> i) & 1) && Cs % 32 == 0;
            st.LC = unpad ? Cs : st.CP; st.L3 = unpad ? 3 * Cs : npad(Cs, st.C3P); st.L4 = unpad ? 4 * Cs : st.C4P;
            st.LD = unpad ? Cs : npad(Cs, st.CP);
        }
        for (SBlock& bk : st.blocks) {
            bk.qkv.out = 3 * Cs; bk.qkv.in = Cs; bk.o.out = Cs; bk.o.in = Cs;
            bk.fc1.out = 4 * Cs; bk.fc1.in = Cs; bk.fc2.out = Cs; bk.fc2.in = 4 * Cs;
            for (SLin* ln : {&bk.qkv, &bk.o, &bk.fc1, &bk.fc2}) {
                A_(ln->W, (size_t)ln->out * ln->in); A_(ln->b, ln->out);
                if (m->f16) {
                    ln->inP = padc(ln->in); ln->outP = padc(ln->out);
                    ln->inN = npad(Cs, ln->inP); ln->outN = npad(Cs, ln->outP);
                    A_(ln->W16, (size_t)ln->outN * ln->inP); A_(ln->WT16, (size_t)ln->inN * ln->outP); A_(ln->b16, ln->outN);
                }
            }
            A_(bk.ln1_g, Cs); A_(bk.ln1_b, Cs); A_(bk.ln2_g, Cs); A_(bk.ln2_b, Cs);
            A_(bk.table, (size_t)(2 * WS - 1) * (2 * WS - 1) * st.heads);
            if (m->r) {
                SLin* lins[6] = {&bk.qkv, &bk.qkv, &bk.qkv, &bk.o, &bk.fc1, &bk.fc2};
                const int rows[6] = {0, Cs, 2 * Cs, 0, 0, 0}, outs[6] = {Cs, Cs, Cs, Cs, 4 * Cs, Cs};
                for (int ti = 0; ti < 6; ++ti) {
                    if (!(cfg->lora_targets & kTargetBits[ti])) continue;
                    SLora sl;
                    sl.row_off = rows[ti]; sl.out = outs[ti]; sl.A = nullptr; sl.B = nullptr;
                    lins[ti]->slots.push_back(sl);
                    off += (int64_t)m->r * lins[ti]->in + (int64_t)sl.out * m->r;
                }
                if (m->f16)
                    for (SLin* ln : {&bk.qkv, &bk.o, &bk.fc1, &bk.fc2}) {
                        if (ln->slots.empty()) continue;
                        ln->kext = 64;
                        A_(ln->Ad, (size_t)64 * ln->inP); A_(ln->Bu, (size_t)ln->outN * 64);
                        A_(ln->Bd, (size_t)64 * ln->outP); A_(ln->Au, (size_t)ln->inN * 64);
                    }
            }
        }
        if (i < 3) {
            A_(st.mg_g, 4 * Cs); A_(st.mg_b, 4 * Cs); A_(st.Wred, (size_t)2 * Cs * 4 * Cs); res /= 2;
            if (m->f16) { A_(st.Wred16, (size_t)padc(2 * Cs) * 4 * Cs); A_(st.WredT16, (size_t)4 * Cs * 2 * Cs); }      // (rows 2C .. of Wred16 stay zero)
        }
    }
    const int Cl = m->E << 3;
    A_(m->fg, Cl); A_(m->fb, Cl); A_(m->Wc, (size_t)m->C * Cl); A_(m->bc, m->C);
    m->flat_n = off;
    A_(m->flat, (size_t)(off > 0 ? off : 4));
#undef A_
    // slot pointers are taken after the vectors stopped growing
    {
        int64_t o2 = 0;
        for (SStage& st : m->stages)
            for (SBlock& bk : st.blocks)
                for (SLin* ln : {&bk.qkv, &bk.o, &bk.fc1, &bk.fc2})
                    for (SLora& sl : ln->slots) {
                        sl.A = m->flat + o2; o2 += (int64_t)m->r * ln->in;
                        sl.B = m->flat + o2; o2 += (int64_t)sl.out * m->r;
                    }
        // NOTE: the loop above visits q, k, v (slots of qkv), o, fc1, fc2 in the same order the offsets were handed out
    }
    if (hipHostMalloc((void**)&m->err_flag, 64, hipHostMallocMapped) != hipSuccess) { vl_swin_destroy(m); return vl_fail(VL_ERR_HIP, "hipHostMalloc failed"); }
    *m->err_flag = 0;
    *out = m;
    return VL_OK;
}

int vl_swin_destroy(vl_swin* m) {
    if (!m) return VL_OK;
    for (hipStream_t sd : m->side) if (sd) (void)hipStreamDestroy(sd);
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    if (m->ev_join) (void)hipEventDestroy(m->ev_join);
    for (void* p : m->allocs) (void)hipFree(p);
    if (m->err_flag) (void)hipHostFree(m->err_flag);
    delete m;
    return VL_OK;
}

// HF-4.55.2 key names of SwinForImageClassification ("swin.encoder.layers.S.blocks.B.attention.self.query.weight", ...)
int vl_swin_load_tensor(vl_swin* m, const char* name, const float* src, int64_t numel, void* stream) {
    if (!m || !name || !src) return vl_fail(VL_ERR_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    auto copyf = [&](float* dst, int64_t n) -> int {
        if (n != numel) return vl_fail(VL_ERR_ARG, "%s: expected %lld elements, got %lld", name, (long long)n, (long long)numel);
        HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        return VL_OK;
    };
    m->dirty = 1;
    const int PK = 3 * m->P * m->P, Cl = m->E << 3;
    if (!strcmp(name, "swin.embeddings.patch_embeddings.projection.weight")) return copyf(m->Wpe, (int64_t)m->E * PK);
    if (!strcmp(name, "swin.embeddings.patch_embeddings.projection.bias")) return copyf(m->bpe, m->E);
    if (!strcmp(name, "swin.embeddings.norm.weight")) return copyf(m->eg, m->E);
    if (!strcmp(name, "swin.embeddings.norm.bias")) return copyf(m->eb, m->E);
    if (!strcmp(name, "swin.layernorm.weight")) return copyf(m->fg, Cl);
    if (!strcmp(name, "swin.layernorm.bias")) return copyf(m->fb, Cl);
    if (!strcmp(name, "classifier.weight")) return copyf(m->Wc, (int64_t)m->C * Cl);
    if (!strcmp(name, "classifier.bias")) return copyf(m->bc, m->C);
    int si = 0, bi = 0;
    const char *rest = nullptr, *rest2 = nullptr;
    if (!parse2(name, "swin.encoder.layers.", &si, &rest) || si < 0 || si > 3) return vl_fail(VL_ERR_ARG, "unknown tensor name: %s", name);
    SStage& st = m->stages[si];
    const int Cs = st.C;
    if (!strcmp(rest, "downsample.norm.weight") && si < 3) return copyf(st.mg_g, 4 * Cs);
    if (!strcmp(rest, "downsample.norm.bias") && si < 3) return copyf(st.mg_b, 4 * Cs);
    if (!strcmp(rest, "downsample.reduction.weight") && si < 3) return copyf(st.Wred, (int64_t)2 * Cs * 4 * Cs);
    if (!parse2(rest, "blocks.", &bi, &rest2) || bi < 0 || bi >= st.depth) return vl_fail(VL_ERR_ARG, "unknown tensor name: %s", name);
    SBlock& bk = st.blocks[bi];
    if (!strcmp(rest2, "layernorm_before.weight")) return copyf(bk.ln1_g, Cs);
    if (!strcmp(rest2, "layernorm_before.bias")) return copyf(bk.ln1_b, Cs);
    if (!strcmp(rest2, "layernorm_after.weight")) return copyf(bk.ln2_g, Cs);
    if (!strcmp(rest2, "layernorm_after.bias")) return copyf(bk.ln2_b, Cs);
    if (!strcmp(rest2, "attention.self.relative_position_bias_table")) return copyf(bk.table, (int64_t)169 * st.heads);
    struct { const char* mod; SLin* ln; int row_off, rows; } mods[6] = {
        {"attention.self.query.", &bk.qkv, 0, Cs}, {"attention.self.key.", &bk.qkv, Cs, Cs}, {"attention.self.value.", &bk.qkv, 2 * Cs, Cs},
        {"attention.output.dense.", &bk.o, 0, Cs}, {"intermediate.dense.", &bk.fc1, 0, 4 * Cs}, {"output.dense.", &bk.fc2, 0, Cs}};
    for (auto& md : mods) {
        const size_t n = strlen(md.mod);
        if (strncmp(rest2, md.mod, n) != 0) continue;
        if (!strcmp(rest2 + n, "weight")) return copyf(md.ln->W + (size_t)md.row_off * md.ln->in, (int64_t)md.rows * md.ln->in);
        if (!strcmp(rest2 + n, "bias")) return copyf(md.ln->b + md.row_off, md.rows);
    }
    return vl_fail(VL_ERR_ARG, "unknown tensor name: %s", name);
}

int vl_swin_param_flat(vl_swin* m, float** ptr, int64_t* numel) {
    if (!m) return vl_fail(VL_ERR_ARG, "null model");
    if (ptr) { *ptr = m->flat; m->dirty = 1; }
    if (numel) *numel = m->flat_n;
    return VL_OK;
}

int vl_swin_param_tensor(vl_swin* m, int stage, int block, uint32_t target, int which, float** ptr, int64_t* numel) {
    if (!m || !ptr || !numel) return vl_fail(VL_ERR_ARG, "null argument");
    if (stage < 0 || stage > 3 || block < 0 || block >= m->stages[stage].depth) return vl_fail(VL_ERR_ARG, "stage / block out of range");
    m->dirty = 1;            // a writable pointer leaves the library
    SBlock& bk = m->stages[stage].blocks[block];
    SLin* lins[6] = {&bk.qkv, &bk.qkv, &bk.qkv, &bk.o, &bk.fc1, &bk.fc2};
    const int Cs = m->stages[stage].C;
    const int rows[6] = {0, Cs, 2 * Cs, 0, 0, 0};
    for (int ti = 0; ti < 6; ++ti) {
        if (kTargetBits[ti] != target) continue;
        for (SLora& sl : lins[ti]->slots)
            if (sl.row_off == rows[ti]) {
                *ptr = which == 0 ? sl.A : sl.B;
                *numel = which == 0 ? (int64_t)m->r * lins[ti]->in : (int64_t)sl.out * m->r;
                return VL_OK;
            }
    }
    return vl_fail(VL_ERR_ARG, "target 0x%x has no adapter", target);
}

int vl_swin_set_normalization(vl_swin* m, const float mean[3], const float stdv[3]) {
    if (!m || !mean || !stdv) return vl_fail(VL_ERR_ARG, "null argument");
    for (int c = 0; c < 3; ++c) { if (!(stdv[c] > 0.f)) return vl_fail(VL_ERR_ARG, "std must be positive"); m->mean[c] = mean[c]; m->stdv[c] = stdv[c]; }
    return VL_OK;
}

// Lays the activations of up to B images out from `base` into `w` (which then holds no forward) and returns the bytes they take;
// base == nullptr: a size query, `w` is a throw-away.
static size_t swin_carve(const vl_swin* m, SwinWs& w, int B, char* base) {
    w.max_batch = base ? B : 0; w.cur_B = 0; w.have_loss = 0;
    Carver cv{base, 0};
    auto take = [&](size_t bytes) { return cv.take<float>(bytes); };
    const int L0 = m->G0 * m->G0, PK = 3 * m->P * m->P;
    const int64_t R0 = round_up((int64_t)B * L0, 64);
    w.patches = take((size_t)R0 * PK * 4);
    if (m->pe16) {       // (rows rounded up to the GEMM's 128-row tiles: the projection reads and stores whole tiles)
        const int64_t R128 = round_up((int64_t)B * L0, 128);
        w.patches16 = (h16*)take((size_t)R128 * PK * 2 + 512); w.emb16 = (h16*)take((size_t)R128 * m->E * 2 + 512);
    }
    w.emb = take((size_t)R0 * m->E * 4); w.emean = take((size_t)R0 * 4); w.erstd = take((size_t)R0 * 4);
    size_t big = 0;
    for (int i = 0; i < 4; ++i) {
        const SStage& st = m->stages[i];
        SStageWs& sw = w.st[i];
        sw.blocks.resize(st.depth);
        const int64_t R = round_up((int64_t)B * st.H * st.H, 512);     // (a quarter of it is still a multiple of the GEMM row tile)
        for (SBlockWs& bw : sw.blocks) {
            bw.mean1 = take((size_t)R * 4); bw.rstd1 = take((size_t)R * 4); bw.mean2 = take((size_t)R * 4); bw.rstd2 = take((size_t)R * 4);
            bw.lse = take((size_t)R * st.heads * 4);
            if (m->f16) continue;              // the 16-bit path keeps its streams and activations as h16 tensors (below)
            bw.xa = take((size_t)R * st.C * 4); bw.xb = take((size_t)R * st.C * 4);
            bw.qkvbuf = take((size_t)R * 3 * st.C * 4); bw.ctx = take((size_t)R * st.C * 4);
            bw.z = take((size_t)R * 4 * st.C * 4);
        }
        if (m->f16) {
            const int64_t Rp = round_up((int64_t)B * st.H * st.H, 128);
            // (+ 512 B: a GEMM whose A rows are narrower than its K reads that far past the last row)
            auto th = [&](size_t n) { return (h16*)take(n * 2 + 512); };
            for (SBlockWs& bw : sw.blocks) {
                bw.qkv16 = th((size_t)Rp * npad(st.C, st.C3P)); bw.z16 = th((size_t)Rp * st.C4P);
                bw.xa16 = th((size_t)Rp * st.C); bw.xb16 = th((size_t)Rp * st.C);
            }
            const size_t CD = (size_t)npad(st.C, st.CP);
            sw.h16b = th((size_t)Rp * st.CP); sw.a16 = th((size_t)Rp * st.C4P); sw.delta16 = th((size_t)Rp * CD);
            sw.ctx16 = th((size_t)Rp * st.CP); sw.t16 = th((size_t)Rp * 64); sw.u16 = th((size_t)Rp * 64);
            sw.dz16 = th((size_t)Rp * st.C4P); sw.dqkv16 = th((size_t)Rp * npad(st.C, st.C3P)); sw.dh16 = th((size_t)Rp * CD);
            sw.dctx16 = th((size_t)Rp * CD); sw.gh16 = th((size_t)Rp * st.CP);
            if (i < 3) { const int64_t Rq = round_up(Rp / 4, 128); sw.mg16 = th((size_t)Rq * 4 * st.C); sw.g16 = th((size_t)Rq * 2 * st.C); }
        }
        if (i < 3) { if (!m->f16) sw.mg = take((size_t)R / 4 * 4 * st.C * 4 + 1024); sw.mmean = take((size_t)R); sw.mrstd = take((size_t)R); }
        if ((size_t)R * 4 * st.C > big) big = (size_t)R * 4 * st.C;
    }
    const int Cl = m->E << 3, Ll = m->stages[3].H * m->stages[3].H;
    w.xlast = take((size_t)round_up((int64_t)B * Ll, 64) * Cl * 4);
    if (m->f16) {
        const size_t nl = (size_t)round_up((int64_t)B * Ll, 64) * Cl * 2;
        w.xlast16 = (h16*)take(nl); w.hfin16 = (h16*)take(nl); w.dhfin16 = (h16*)take(nl);
    }
    w.fmean = take((size_t)B * Ll * 4 + 256); w.frstd = take((size_t)B * Ll * 4 + 256);
    w.hfin = take((size_t)round_up((int64_t)B * Ll, 64) * Cl * 4);
    w.pooled = take((size_t)B * Cl * 4); w.dpooled = take((size_t)B * Cl * 4);
    w.logits = take((size_t)B * m->C * 4); w.dlogits = take((size_t)B * m->C * 4);
    w.loss = take(256); w.loss_img = take((size_t)B * 4);
    w.gscale = take((size_t)B * 4); w.inv_gscale = take((size_t)B * 4); w.dlogits_s = take((size_t)B * m->C * 4);
    if (m->f16) big = 64;       // the 16-bit path has no fp32 activation scratch (round 5: h16 streams); g1 serves the embedding backward
    w.h = take(big * 4); w.a = take(big * 4); w.dbig = take(big * 4);
    w.dqkv = take(big * 4);
    w.t = take((size_t)R0 * 64 * 4); w.u = take((size_t)R0 * 64 * 4);
    w.g0 = take((size_t)R0 * m->E * 4 + big); w.g1 = take((size_t)R0 * m->E * 4 + big);
    const size_t img = (size_t)B * 3 * m->S * m->S * 4;
    w.grad_img = take(img); w.stage_x0 = take(img); w.stage_adv = take(img);
    w.stage_labels = (int64_t*)take((size_t)B * 8);
    return cv.off;
}

// chain workspaces: each for ceil(max_batch / 2) images, carved into the same bytes as the main workspace
static int swin_chain_images(const vl_swin* m, int max_batch) {
    const int nc = m->chains_on;
    return (m->f16 && nc >= 2 && max_batch >= m->chain_min && max_batch >= nc) ? (max_batch + nc - 1) / nc : 0;
}
static size_t swin_plan_bytes(const vl_swin* m, int max_batch) {
    SwinWs scratch;
    const size_t main_need = swin_carve(m, scratch, max_batch, nullptr);
    const int cb = swin_chain_images(m, max_batch);
    return cb ? std::max(main_need, (size_t)m->chains_on * swin_carve(m, scratch, cb, nullptr)) : main_need;
}

int vl_swin_plan(vl_swin* m, int max_batch, size_t* bytes) {
    if (!m || !bytes || max_batch <= 0) return vl_fail(VL_ERR_ARG, "bad argument");
    if (m->f16) {
        // 32-bit byte offsets inside an operand (as the ViT path): stage 0's [B * 56 * 56, 4 C] h16 activation must stay below 4 GiB
        const SStage& s0 = m->stages[0];
        const int64_t rows = round_up((int64_t)max_batch * s0.H * s0.H, 512), wide = round_up(4 * (int64_t)s0.C, 128);
        if (rows * wide >= ((int64_t)1 << 31))
            return vl_fail(VL_ERR_UNSUPPORTED, "max_batch %d: an activation of %lld x %lld 16-bit elements exceeds the 4 GiB the kernels' "
                           "32-bit operand offsets reach; split the batch", max_batch, (long long)rows, (long long)wide);
    }
    *bytes = swin_plan_bytes(m, max_batch);
    m->w.max_batch = -max_batch;       // planned, not armed
    return VL_OK;
}

int vl_swin_set_workspace(vl_swin* m, void* ws, size_t bytes) {
    if (!m || !ws) return vl_fail(VL_ERR_ARG, "null argument");
    if (m->w.max_batch >= 0) return vl_fail(VL_ERR_STATE, "vl_swin_set_workspace before vl_swin_plan");
    const int B = -m->w.max_batch;
    if (((uintptr_t)ws) & 255) return vl_fail(VL_ERR_ARG, "workspace must be 256-byte aligned");
    const size_t need = swin_plan_bytes(m, B);
    if (bytes < need) return vl_fail(VL_ERR_ARG, "workspace too small: %zu < %zu", bytes, need);
    if (hipMemset(ws, 0, need) != hipSuccess) return vl_fail(VL_ERR_HIP, "hipMemset(workspace) failed");
    swin_carve(m, m->w, B, (char*)ws);
    m->chain_batch = swin_chain_images(m, B);
    if (const int cb = m->chain_batch) {
        size_t one = 0;       // chain c at offset c * one of the same bytes
        for (int c = 0; c < m->chains_on; ++c) one = swin_carve(m, m->chain[c], cb, (char*)ws + (size_t)c * one);
        for (int k = 0; k + 1 < m->chains_on; ++k)
            if (!m->side[k]) HIPCHK(hipStreamCreateWithFlags(&m->side[k], hipStreamNonBlocking));
        if (!m->ev_fork) HIPCHK(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
        if (!m->ev_join) HIPCHK(hipEventCreateWithFlags(&m->ev_join, hipEventDisableTiming));
    }
    return VL_OK;
}

static int swin_forward(vl_swin* m, SwinWs& w, const float* x, int B, int normalise, hipStream_t s) {
    if (B <= 0 || B > w.max_batch) return vl_fail(VL_ERR_STATE, "batch %d exceeds planned workspace (%d)", B, w.max_batch);
    const int L0 = m->G0 * m->G0, PK = 3 * m->P * m->P;
    if (m->f16 && m->dirty) swin16_commit(m, s);
    // patch embedding: Conv2d(3, E, k = s = P) as a GEMM over gathered patches, then LayerNorm (SwinEmbeddings)
    if (m->f16) {   // K-tail heads of the unpadded stages' GEMM A operands (zero_tails_kernel)
            TailPtrs tp; tp.n = 0;
            for (int i = 0; i < 4; ++i) {
                const SStage& st = m->stages[i];
                const SStageWs& sw = w.st[i];
                const int64_t Mi = (int64_t)B * st.H * st.H;
                if (st.LC < st.CP) { tp.p[tp.n++] = sw.h16b + Mi * st.LC; tp.p[tp.n++] = sw.ctx16 + Mi * st.LC; tp.p[tp.n++] = sw.gh16 + Mi * st.LC; }
                if (st.L3 < st.C3P) tp.p[tp.n++] = sw.dqkv16 + Mi * st.L3;
            }
            if (m->pe16) {      // patches (48 of the 64-deep K tile)
                tp.p[tp.n++] = w.patches16 + (int64_t)B * L0 * PK;
                // (the embedding gradient is staged in stage 1's h16b -- never a GEMM result, so its pad rows hold nothing but these zeros)
            }
            if (tp.n) hipLaunchKernelGGL(zero_tails_kernel, dim3(tp.n), dim3(64), 0, s, tp);
        }
    if (m->pe16) {
        // 16-bit patch embedding: h16 patches [B L0][48] (K tail of the 64-deep tile read from the next row against zero weight
        // columns), projection on the streaming GEMM, h16 result of width E
        hipLaunchKernelGGL(patch_gather16_p4_kernel, dim3(nblk((int64_t)B * L0 * 6, 256, 8192)), dim3(256), 0, s, x, w.patches16, B, m->S, m->G0,
                           normalise, m->mean[0], m->mean[1], m->mean[2], 1.f / m->stdv[0], 1.f / m->stdv[1], 1.f / m->stdv[2]);
        GemmArgs ge = ga(w.patches16, PK, m->Wpe16, 64, 64, (int)round_up((int64_t)B * L0, 128), 128);
        ge.Mvalid = B * L0; ge.bias = m->bpe16; ge.C = w.emb16; ge.ldc = m->E; ge.n_store = m->E; ge.n_algo = m->E;
        launch_gemm(ge, EPI_STORE_H16, 128, s);
    } else {
    k_patch_gather_f32(x, w.patches, B, m->S, m->P, normalise, m->mean, m->stdv, s);
    GemmF32 g = gm(w.patches, PK, m->Wpe, PK, 0, B * L0, m->E, PK, w.emb, m->E);
    g.bias = m->bpe;
    k_gemm_f32(g, s);
    }
    if (m->f16) {
        // ---- 16-bit path (round 5: h16 residual streams; the embedding LayerNorm's output IS the stream of stage 1) ----
        if (m->pe16) sw_ln_fwd16<false>(w.emb16, m->E, nullptr, 0, nullptr, 0, w.st[0].blocks[0].xa16, m->E, w.emean, w.erstd, m->eg,
                                        m->eb, B * L0, m->E, m->cfg.ln_eps, m->err_flag, s);
        else
        sw_ln_fwd16<true>(w.emb, m->E, nullptr, 0, nullptr, 0, w.st[0].blocks[0].xa16, m->E, w.emean, w.erstd, m->eg, m->eb,
                          B * L0, m->E, m->cfg.ln_eps, m->err_flag, s);
        for (int i = 0; i < 4; ++i) {
            const SStage& st = m->stages[i];
            SStageWs& sw = w.st[i];
            const int Cs = st.C, Hs = st.H, M = B * Hs * Hs;
            // the stream leaves a block as {bw.xb16, sw.delta16}: the next LayerNorm adds them
            for (int bi = 0; bi < st.depth; ++bi) {
                const int shift = (bi & 1) && Hs > WS ? WS / 2 : 0;          // SwinLayer: no shift when the window covers the map
                swin16_block_fwd(m, st, sw, st.blocks[bi], sw.blocks[bi], bi ? sw.blocks[bi - 1].xb16 : nullptr, bi > 0, B, shift, s);
            }
            const SBlockWs& last = sw.blocks[st.depth - 1];
            if (i == 3) {
                // stage output x' = round16(xb + delta) -> xlast16, and the final LayerNorm over every token in the same pass
                sw_ln_fwd16<false>(last.xb16, Cs, sw.delta16, st.LD, w.xlast16, Cs, w.hfin16, Cs, w.fmean, w.frstd, m->fg, m->fb, M, Cs,
                                   m->cfg.ln_eps, m->err_flag, s);
                break;
            }
            // SwinPatchMerging: gather + LayerNorm(4C) in one pass over {xb16, delta16}; the reduction (no bias) on h16 operands
            // writes the next stage's stream, its rows narrower than the tile grid where 2C is not a multiple of 128
            const int Mq = (int)round_up(M / 4, 128), N2 = padc(2 * Cs);
            merge_dispatch(Cs, [&](auto nv, auto gl) {
                constexpr int NV = decltype(nv)::value, GL = decltype(gl)::value;
                hipLaunchKernelGGL((merge_ln_fwd16_kernel<NV, GL>), dim3((M / 4 + 4 * (64 / GL) - 1) / (4 * (64 / GL))), dim3(256), 0, s,
                                   last.xb16, sw.delta16, st.LD, sw.mg16, sw.mmean, sw.mrstd, st.mg_g, st.mg_b, B, Hs, Hs, Cs, m->cfg.ln_eps);
            });
            GemmArgs g16a = ga(sw.mg16, 4 * Cs, st.Wred16, 4 * Cs, 4 * Cs, Mq, N2);
            g16a.Mvalid = M / 4; g16a.C = w.st[i + 1].blocks[0].xa16; g16a.ldc = 2 * Cs; g16a.n_store = N2 > 2 * Cs ? 2 * Cs : 0;
            launch_gemm(g16a, EPI_STORE_H16, 128, s);
        }
        const int Cl = m->E << 3, Ll = m->stages[3].H * m->stages[3].H;
        hipLaunchKernelGGL(mean_pool16_kernel, dim3(nblk((int64_t)B * Cl, 256, 1 << 30)), dim3(256), 0, s, w.hfin16, w.pooled, B, Ll, Cl);
        hipLaunchKernelGGL(cls_fwd_kernel, dim3(nblk((int64_t)B * m->C, 4, 1 << 30)), dim3(256), 0, s, w.pooled, m->Wc, m->bc, w.logits, B,
                           m->C, Cl);
        w.cur_B = B; w.cur_norm = normalise; w.have_loss = 0;
        return VL_OK;
    }
    k_ln_fwd_f32(w.emb, w.st[0].blocks[0].xa, w.emean, w.erstd, m->eg, m->eb, B * L0, m->E, m->cfg.ln_eps, s);
    for (int i = 0; i < 4; ++i) {
        const SStage& st = m->stages[i];
        SStageWs& sw = w.st[i];
        const int Cs = st.C, Hs = st.H, M = B * Hs * Hs;
        const int nW = (Hs / WS) * (Hs / WS);
        for (int bi = 0; bi < st.depth; ++bi) {
            const SBlock& bk = st.blocks[bi];
            SBlockWs& bw = sw.blocks[bi];
            const int shift = (bi & 1) && Hs > WS ? WS / 2 : 0;          // SwinLayer: no shift when the window covers the map
            float* xout = bi + 1 < st.depth ? sw.blocks[bi + 1].xa : (i < 3 ? w.dbig : w.xlast);
            k_ln_fwd_f32(bw.xa, w.h, bw.mean1, bw.rstd1, bk.ln1_g, bk.ln1_b, M, Cs, m->cfg.ln_eps, s);
            lin_fwd(m, w, bk.qkv, w.h, M, bw.qkvbuf, nullptr, s);
            if (g_poison_lds) vl_poison_lds(s);      // test hook (prof.h): the window kernels keep K / V / Q / dO of a window in LDS
            hipLaunchKernelGGL(win_attn_fwd_kernel, dim3(nblk((int64_t)B * nW * st.heads, 4, 1 << 30)), dim3(256), 0, s, bw.qkvbuf,
                               bk.table, bw.ctx, bw.lse, B, Hs, Hs, Cs, st.heads, shift);
            lin_fwd(m, w, bk.o, bw.ctx, M, bw.xb, bw.xa, s);
            k_ln_fwd_f32(bw.xb, w.h, bw.mean2, bw.rstd2, bk.ln2_g, bk.ln2_b, M, Cs, m->cfg.ln_eps, s);
            lin_fwd(m, w, bk.fc1, w.h, M, bw.z, nullptr, s);
            k_gelu_fwd_f32(bw.z, w.a, (int64_t)M * 4 * Cs, s);
            lin_fwd(m, w, bk.fc2, w.a, M, xout, bw.xb, s);
        }
        if (i < 3) {        // SwinPatchMerging: 2x2 neighbourhood -> 4C, LayerNorm, Linear(4C -> 2C, no bias)
            hipLaunchKernelGGL(merge_gather_kernel, dim3(nblk((int64_t)M * Cs, 256, 8192)), dim3(256), 0, s, w.dbig, sw.mg, B, Hs,
                               Hs, Cs, 0);
            k_ln_fwd_f32(sw.mg, w.h, sw.mmean, sw.mrstd, st.mg_g, st.mg_b, M / 4, 4 * Cs, m->cfg.ln_eps, s);
            k_gemm_f32(gm(w.h, 4 * Cs, st.Wred, 4 * Cs, 0, M / 4, 2 * Cs, 4 * Cs, w.st[i + 1].blocks[0].xa, 2 * Cs), s);
        }
    }
    // final LayerNorm over every token, mean pool, classifier (SwinModel.pooler + SwinForImageClassification.classifier)
    const int Cl = m->E << 3, Ll = m->stages[3].H * m->stages[3].H;
    k_ln_fwd_f32(w.xlast, w.hfin, w.fmean, w.frstd, m->fg, m->fb, B * Ll, Cl, m->cfg.ln_eps, s);
    hipLaunchKernelGGL(mean_pool_kernel, dim3(nblk((int64_t)B * Cl, 256, 1 << 30)), dim3(256), 0, s, w.hfin, w.pooled, B, Ll, Cl);
    hipLaunchKernelGGL(cls_fwd_kernel, dim3(nblk((int64_t)B * m->C, 4, 1 << 30)), dim3(256), 0, s, w.pooled, m->Wc, m->bc, w.logits, B,
                       m->C, Cl);
    w.cur_B = B; w.cur_norm = normalise; w.have_loss = 0;
    return VL_OK;
}

static int swin_backward(const vl_swin* m, SwinWs& w, float* grad_x, hipStream_t s) {
    if (!w.have_loss) return vl_fail(VL_ERR_STATE, "backward before vl_swin_loss_ce");
    const int B = w.cur_B;
    const int Cl = m->E << 3, Ll = m->stages[3].H * m->stages[3].H;
    // head: d(pooled) = dlogits Wc ; d(hfin)[b, t] = d(pooled)[b] / L ; LayerNorm backward
    const float* dlog = w.dlogits;
    if (m->f16) {
        // per-image power-of-two scale: the largest |dLoss/dlogits| of an image lands in [2^9, 2^10) (as the ViT 16-bit path;
        // the chain is linear and per image, so it is exact up to under / overflow and is undone at the pixels)
        k_grad_scale(w.dlogits, B, m->C, 0, w.gscale, w.inv_gscale, s);
        hipLaunchKernelGGL(scale_rows_kernel, dim3(nblk((int64_t)B * m->C, 256, 1024)), dim3(256), 0, s, w.dlogits, w.gscale, w.dlogits_s, B, (int64_t)m->C);
        dlog = w.dlogits_s;
    }
    hipLaunchKernelGGL(cls_bwd_kernel, dim3(nblk((int64_t)B * Cl, 256, 1 << 30)), dim3(256), 0, s, dlog, m->Wc, w.dpooled, B, m->C, Cl);
    if (m->f16) {
        // ---- 16-bit path: ONE h16 gradient stream per stage (sw.gh16, row stride st.LC), updated in place by every LayerNorm
        // backward and read as the A operand of the dgrad GEMMs (round 5; the fp32 stream + h16 shadow of round 3 are gone) ----
        hipLaunchKernelGGL(mean_pool_bwd16_kernel, dim3(nblk((int64_t)B * Ll * Cl, 256, 1 << 30)), dim3(256), 0, s, w.dpooled, w.dhfin16, B, Ll, Cl);
        sw_ln_bwd16<false, false>(w.dhfin16, Cl, w.xlast16, Cl, w.fmean, w.frstd, m->fg, nullptr, w.st[3].gh16, m->stages[3].LC,
                                  B * Ll, Cl, m->err_flag, s);
        for (int i = 3; i >= 0; --i) {
            const SStage& st = m->stages[i];
            SStageWs& sw = w.st[i];
            const int Cs = st.C, Hs = st.H, M = B * Hs * Hs;
            if (i < 3) {
                // the next stage's gradient stream [M/4, 2C] -> reduction dgrad (h16 result in sw.mg16, free in the backward) ->
                // LayerNorm(4C) backward with x gathered again from {xb16, delta16}, un-merged on the way out into sw.gh16
                const SStage& nx = m->stages[i + 1];
                const int Mq = (int)round_up(M / 4, 128);
                GemmArgs g16a = ga(w.st[i + 1].gh16, nx.LC, st.WredT16, 2 * Cs, 2 * Cs, Mq, 4 * Cs);
                g16a.Mvalid = M / 4; g16a.C = sw.mg16; g16a.ldc = 4 * Cs;
                launch_gemm(g16a, EPI_STORE_H16, 128, s);
                merge_dispatch(Cs, [&](auto nv, auto gl) {
                    constexpr int NV = decltype(nv)::value, GL = decltype(gl)::value;
                    hipLaunchKernelGGL((merge_ln_bwd16_kernel<NV, GL>), dim3((M / 4 + 4 * (64 / GL) - 1) / (4 * (64 / GL))), dim3(256), 0, s,
                                       sw.mg16, sw.blocks[st.depth - 1].xb16, sw.delta16, st.LD, sw.mmean, sw.mrstd, st.mg_g, sw.gh16,
                                       st.LC, B, Hs, Hs, Cs, m->err_flag);
                });
            }
            for (int bi = st.depth - 1; bi >= 0; --bi) {
                const int shift = (bi & 1) && Hs > WS ? WS / 2 : 0;
                swin16_block_bwd(m, st, sw, st.blocks[bi], sw.blocks[bi], B, shift, s);
            }
        }
        if (grad_x) {
            const int L0 = m->G0 * m->G0, PK = 3 * m->P * m->P;
            // embedding LayerNorm backward (x = the fp32 patch-embedding output) -> fp32, then the patch projection's dgrad in fp32
            float is[3];
            for (int c = 0; c < 3; ++c) is[c] = w.cur_norm ? 1.f / m->stdv[c] : 1.f;
            if (m->pe16) {
                // embedding LayerNorm backward on h16 (its result in stage 1's h16b, free by now), the projection's dgrad on the
                // streaming GEMM (h16 d(patches) over the forward's patches), then ONE scatter to pixels that also undoes the scale
                h16* gemb = w.st[0].h16b;       // (a LayerNorm-output buffer: rows >= M are never written, its K-tail head is zeroed per forward)
                sw_ln_bwd16<false, false>(w.st[0].gh16, m->stages[0].LC, w.emb16, m->E, w.emean, w.erstd, m->eg, nullptr, gemb, m->E,
                                          B * L0, m->E, m->err_flag, s);
                GemmArgs gd = ga(gemb, m->E, m->WpeT16, 128, 128, (int)round_up((int64_t)B * L0, 128), 128);
                gd.Mvalid = B * L0; gd.C = w.patches16; gd.ldc = PK; gd.n_store = PK; gd.n_algo = PK;
                launch_gemm(gd, EPI_STORE_H16, 128, s);
                hipLaunchKernelGGL(patch_scatter16_p4_kernel, dim3(nblk((int64_t)B * L0 * 6, 256, 8192)), dim3(256), 0, s, w.patches16, grad_x, B, m->S,
                                   m->G0, is[0], is[1], is[2], w.inv_gscale, m->err_flag);
                return VL_OK;
            }
            sw_ln_bwd16<true, true>(w.st[0].gh16, m->stages[0].LC, w.emb, m->E, w.emean, w.erstd, m->eg, nullptr, w.g1, m->E,
                                    B * L0, m->E, m->err_flag, s);
            k_gemm_f32(gm(w.g1, m->E, m->Wpe, PK, 1, B * L0, PK, m->E, w.patches, PK), s);
            k_patch_scatter_f32(w.patches, grad_x, B, m->S, m->P, is, s);
            // undo the per-image gradient scale
            hipLaunchKernelGGL(scale_rows_kernel, dim3(8192), dim3(256), 0, s, grad_x, w.inv_gscale, grad_x, B, (int64_t)3 * m->S * m->S);
        }
        return VL_OK;
    }
    hipLaunchKernelGGL(mean_pool_bwd_kernel, dim3(nblk((int64_t)B * Ll * Cl, 256, 1 << 30)), dim3(256), 0, s, w.dpooled, w.h, B, Ll, Cl);
    float *gcur = w.g0, *gnext = w.g1;
    k_ln_bwd_f32(w.h, w.xlast, w.fmean, w.frstd, m->fg, nullptr, gcur, B * Ll, Cl, s);
    for (int i = 3; i >= 0; --i) {
        const SStage& st = m->stages[i];
        SStageWs& sw = w.st[i];
        const int Cs = st.C, Hs = st.H, M = B * Hs * Hs;
        const int nW = (Hs / WS) * (Hs / WS);
        if (i < 3) {
            // gcur = gradient w.r.t. the next stage's input [M/4, 2C]: reduction dgrad, LayerNorm backward, un-merge
            k_gemm_f32(gm(gcur, 2 * Cs, st.Wred, 4 * Cs, 1, M / 4, 4 * Cs, 2 * Cs, w.dbig, 4 * Cs), s);
            k_ln_bwd_f32(w.dbig, sw.mg, sw.mmean, sw.mrstd, st.mg_g, nullptr, w.h, M / 4, 4 * Cs, s);
            hipLaunchKernelGGL(merge_gather_kernel, dim3(nblk((int64_t)M * Cs, 256, 8192)), dim3(256), 0, s, w.h, gcur, B, Hs, Hs, Cs, 1);
        }
        for (int bi = st.depth - 1; bi >= 0; --bi) {
            const SBlock& bk = st.blocks[bi];
            SBlockWs& bw = sw.blocks[bi];
            const int shift = (bi & 1) && Hs > WS ? WS / 2 : 0;
            lin_dgrad(m, w, bk.fc2, gcur, M, w.dbig, s);                                   // d(a)
            k_gelu_bwd_f32(w.dbig, bw.z, (int64_t)M * 4 * Cs, s);                       // d(z)
            lin_dgrad(m, w, bk.fc1, w.dbig, M, w.h, s);
            k_ln_bwd_f32(w.h, bw.xb, bw.mean2, bw.rstd2, bk.ln2_g, gcur, gnext, M, Cs, s);
            lin_dgrad(m, w, bk.o, gnext, M, w.a, s);                                       // d(ctx)
            if (g_poison_lds) vl_poison_lds(s);      // test hook (prof.h): the window kernels keep K / V / Q / dO of a window in LDS
            hipLaunchKernelGGL(win_attn_bwd_kernel, dim3(nblk((int64_t)B * nW * st.heads, 2, 1 << 30)), dim3(128), 0, s, bw.qkvbuf,
                               bk.table, bw.ctx, w.a, bw.lse, w.dqkv, B, Hs, Hs, Cs, st.heads, shift);
            lin_dgrad(m, w, bk.qkv, w.dqkv, M, w.h, s);
            k_ln_bwd_f32(w.h, bw.xa, bw.mean1, bw.rstd1, bk.ln1_g, gnext, gcur, M, Cs, s);
        }
    }
    if (grad_x) {
        const int L0 = m->G0 * m->G0, PK = 3 * m->P * m->P;
        k_ln_bwd_f32(gcur, w.emb, w.emean, w.erstd, m->eg, nullptr, gnext, B * L0, m->E, s);
        k_gemm_f32(gm(gnext, m->E, m->Wpe, PK, 1, B * L0, PK, m->E, w.patches, PK), s);
        float is[3];
        for (int c = 0; c < 3; ++c) is[c] = w.cur_norm ? 1.f / m->stdv[c] : 1.f;
        k_patch_scatter_f32(w.patches, grad_x, B, m->S, m->P, is, s);
    }
    return VL_OK;
}

// the pinned host word kernels write: 1 = bad label (k_ce_loss), 2 = an fp16-mode gradient left its range / is NaN (LayerNorm
// and merge backward, the PGD step), like check_async of the ViT handle
static int swin_check(vl_swin* m) {
    if (m->err_flag && *m->err_flag) {
        const int code = *m->err_flag;
        *m->err_flag = 0;
        if (code == 1) return vl_fail(VL_ERR_ARG, "a label passed to an earlier call was outside [0, num_labels)");
        if (code == 2 || code == 3)
            return vl_fail(VL_ERR_NONFINITE, "an earlier backward pass produced a non-finite input gradient (fp16 range exceeded): "
                                             "redo that batch with precision = f32");
        return vl_fail(VL_ERR_HIP, "device-side error flag %d", code);
    }
    return VL_OK;
}
static int swin_launch_ok(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vl_fail(VL_ERR_HIP, "%s: kernel launch failed: %s", what, hipGetErrorString(e));
    return VL_OK;
}

int vl_swin_forward(vl_swin* m, const float* x, int batch, int normalise, float* logits_out, void* stream) {
    if (!m || !x) return vl_fail(VL_ERR_ARG, "null argument");
    if (m->w.max_batch <= 0) return vl_fail(VL_ERR_STATE, "no workspace: call vl_swin_plan + vl_swin_set_workspace first");
    int rc = swin_check(m);
    if (rc) return rc;
    if ((rc = swin_forward(m, m->w, x, batch, normalise, (hipStream_t)stream))) return rc;
    if (logits_out) HIPCHK(hipMemcpyAsync(logits_out, m->w.logits, (size_t)batch * m->C * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return swin_launch_ok("vl_swin_forward");
}

int vl_swin_loss_ce(vl_swin* m, const int64_t* labels, float* loss_out, void* stream) {
    if (!m || !labels) return vl_fail(VL_ERR_ARG, "null argument");
    SwinWs& w = m->w;
    if (!w.cur_B) return vl_fail(VL_ERR_STATE, "vl_swin_loss_ce before vl_swin_forward");
    k_ce_loss(w.logits, labels, w.cur_B, m->C, w.dlogits, w.loss_img, w.loss, m->err_flag, (hipStream_t)stream);
    if (loss_out) HIPCHK(hipMemcpyAsync(loss_out, w.loss, sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    w.have_loss = 1;
    return VL_OK;
}

int vl_swin_backward_input(vl_swin* m, float* grad_x_out, void* stream) {
    if (!m || !grad_x_out) return vl_fail(VL_ERR_ARG, "null argument");
    int rc = swin_check(m);
    if (rc) return rc;
    if ((rc = swin_backward(m, m->w, grad_x_out, (hipStream_t)stream))) return rc;
    return swin_launch_ok("vl_swin_backward_input");
}

int vl_swin_pgd_attack(vl_swin* m, const float* x0, const int64_t* labels, int batch, float eps, float alpha, int steps,
                       int random_start, uint64_t seed, float* adv_out, void* stream) {
    if (!m || !x0 || !labels || !adv_out) return vl_fail(VL_ERR_ARG, "bad argument");
    SwinWs& w = m->w;
    if (w.max_batch <= 0 || batch <= 0 || batch > w.max_batch) return vl_fail(VL_ERR_STATE, "batch exceeds planned workspace");
    hipStream_t s = (hipStream_t)stream;
    int rc = swin_check(m);
    if (rc) return rc;
    const int64_t n = (int64_t)batch * 3 * m->S * m->S;
    if (m->chain_batch && batch >= m->chain_min && batch >= m->chains_on && steps > 0) {
        // ---- two half-batch chains (see the handle): images are independent, chain c runs in workspace m->chain[c] on s / a side stream ----
        const int NC = m->chains_on;
        int bsz[vl_swin::MAXCH], first[vl_swin::MAXCH];
        for (int c = 0, at = 0; c < NC; ++c) { bsz[c] = batch / NC + (c < batch % NC ? 1 : 0); first[c] = at; at += bsz[c]; }
        const int64_t img = (int64_t)3 * m->S * m->S;
        if (m->f16 && m->dirty) { swin16_commit(m, s); }
        for (int c = 0; c < NC; ++c) {
            SwinWs& ch = m->chain[c];
            HIPCHK(hipMemcpyAsync(ch.stage_x0, x0 + first[c] * img, (size_t)bsz[c] * img * sizeof(float), hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(ch.stage_labels, labels + first[c], (size_t)bsz[c] * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        }
        // the random start is a function of (seed, element index of the WHOLE batch): drawn once into the caller's buffer
        if (random_start) k_pgd_init(adv_out, x0, eps, 0.f, 1.f, seed, n, s);
        else if (adv_out != x0) HIPCHK(hipMemcpyAsync(adv_out, x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        for (int c = 0; c < NC; ++c)
            HIPCHK(hipMemcpyAsync(m->chain[c].stage_adv, adv_out + first[c] * img, (size_t)bsz[c] * img * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHK(hipEventRecord(m->ev_fork, s));
        for (int c = 1; c < NC; ++c) HIPCHK(hipStreamWaitEvent(m->side[c - 1], m->ev_fork, 0));
        for (int i = 0; i < steps; ++i)
            for (int c = 0; c < NC; ++c) {
                SwinWs& ch = m->chain[c];
                hipStream_t sc = c ? m->side[c - 1] : s;
                const int64_t nc = (int64_t)bsz[c] * img;
                if ((rc = swin_forward(m, ch, ch.stage_adv, bsz[c], 1, sc))) return rc;
                k_ce_loss(ch.logits, ch.stage_labels, bsz[c], m->C, ch.dlogits, ch.loss_img, ch.loss, m->err_flag, sc);
                ch.have_loss = 1;
                if ((rc = swin_backward(m, ch, ch.grad_img, sc))) return rc;
                k_pgd_step(ch.stage_adv, ch.stage_x0, ch.grad_img, eps, alpha, 0.f, 1.f, nc, sc, m->err_flag);
            }
        for (int c = 1; c < NC; ++c) {
            HIPCHK(hipEventRecord(m->ev_join, m->side[c - 1]));
            HIPCHK(hipStreamWaitEvent(s, m->ev_join, 0));
        }
        for (int c = 0; c < NC; ++c)
            HIPCHK(hipMemcpyAsync(adv_out + first[c] * img, m->chain[c].stage_adv, (size_t)bsz[c] * img * sizeof(float), hipMemcpyDeviceToDevice, s));
        w.cur_B = 0; w.have_loss = 0;        // the main workspace shares its bytes with the chains: no forward of the whole batch is held
        return swin_launch_ok("vl_swin_pgd_attack");
    }
    HIPCHK(hipMemcpyAsync(w.stage_x0, x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(w.stage_labels, labels, (size_t)batch * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    if (random_start) k_pgd_init(w.stage_adv, w.stage_x0, eps, 0.f, 1.f, seed, n, s);
    else HIPCHK(hipMemcpyAsync(w.stage_adv, w.stage_x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (int i = 0; i < steps; ++i) {
        if ((rc = swin_forward(m, w, w.stage_adv, batch, 1, s))) return rc;
        k_ce_loss(w.logits, w.stage_labels, batch, m->C, w.dlogits, w.loss_img, w.loss, m->err_flag, s);
        w.have_loss = 1;
        if ((rc = swin_backward(m, w, w.grad_img, s))) return rc;
        k_pgd_step(w.stage_adv, w.stage_x0, w.grad_img, eps, alpha, 0.f, 1.f, n, s, m->err_flag);
    }
    HIPCHK(hipMemcpyAsync(adv_out, w.stage_adv, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return swin_launch_ok("vl_swin_pgd_attack");
}

// vl_check_errors for a Swin handle: synchronises `stream` and reports what the kernels enqueued so far flagged
int vl_swin_check_errors(vl_swin* m, void* stream) {
    if (!m) return vl_fail(VL_ERR_ARG, "null model");
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return vl_fail(VL_ERR_HIP, "hipStreamSynchronize failed");
    return swin_check(m);
}

}  // extern "C"

}  // namespace VLNS
