// What libvitlora_hip.so holds ONCE, whatever the operand type (build.sh compiles this file once; the 16-bit path is compiled
// twice: common.h): the process-wide state -- profiler, LDS-poison test hook, the list of live handles, the last error text --
// and the entry points of include/vitlora.h that take no handle and launch a kernel of once_kernels.hip.  Host-side only, but
// for the poison kernel; the handle-less entry points of the adversarial patch are in patch.hip, beside their kernels.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "model.h"
#include "prof.h"

using namespace vl_once;
#define fail vl_fail

Profiler* g_prof = nullptr;
int g_poison_lds = 0;
long long g_poison_count = 0;
namespace {
__global__ __launch_bounds__(256) void poison_lds_kernel(unsigned pattern, unsigned* sink) {
    extern __shared__ unsigned lds_all[];
    constexpr int N = 160 * 1024 / 4;
    for (int i = threadIdx.x; i < N; i += 256) lds_all[i] = pattern;
    __syncthreads();
    if (sink && lds_all[(threadIdx.x * 97) % N] != pattern) *sink = 1;      // keeps the stores alive
}
}  // namespace
void vl_poison_lds(hipStream_t s) {
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void*)poison_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; }
    int dev = 0, cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    // one workgroup owns a CU's whole LDS, so 2 x #CUs workgroups reach every CU of an otherwise idle stream
    hipLaunchKernelGGL(poison_lds_kernel, dim3(2 * cus), dim3(256), 160 * 1024, s, 0xFFFFFFFFu, (unsigned*)nullptr);
    if (hipGetLastError() == hipSuccess) ++g_poison_count;
}
std::vector<VlFlatRecord> g_vl_models;
namespace {
thread_local std::string g_err;
}

int vl_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" {

const char* vl_version(void) { return "vitlora-hip 0.3 (gfx950; fp16 / bf16 operands or fp32)"; }
const char* vl_last_error(void) { return g_err.c_str(); }

// ---- the attacks' kernels on caller-owned buffers (the attacks themselves: vit_attacks.hip) ----
int vl_pgd_step(float* adv, const float* x0, const float* grad, float eps, float alpha, float lo, float hi, int64_t n, void* stream) {
    if (!adv || !x0 || !grad || n <= 0) return fail(VL_ERR_ARG, "bad argument");
    k_pgd_step(adv, x0, grad, eps, alpha, lo, hi, n, (hipStream_t)stream);
    return VL_OK;
}

int vl_pgd_init(float* adv, const float* x0, float eps, float lo, float hi, uint64_t seed, int64_t n, void* stream) {
    if (!adv || !x0 || n <= 0) return fail(VL_ERR_ARG, "bad argument");
    k_pgd_init(adv, x0, eps, lo, hi, seed, n, (hipStream_t)stream);
    return VL_OK;
}

int vl_dlr_targeted_loss(const float* logits, const int64_t* labels, const int32_t* targets, int B, int C, float* loss_img,
                         float* dlogits, int* err_flag, void* stream) {
    if (!logits || !labels || !targets || !loss_img || !dlogits || B <= 0) return fail(VL_ERR_ARG, "bad argument");
    if (C < 4) return fail(VL_ERR_UNSUPPORTED, "the DLR loss needs at least 4 classes");
    k_dlr_targeted_loss(logits, labels, targets, B, C, dlogits, loss_img, nullptr, err_flag, (hipStream_t)stream);
    return VL_OK;
}

int vl_apgd_targets(const float* logits, const int64_t* labels, int B, int C, int n_target, int32_t* targets,
                    int32_t* clean_correct, void* stream) {
    if (!logits || !labels || !targets || !clean_correct || B <= 0 || C < 2) return fail(VL_ERR_ARG, "bad argument");
    if (n_target < 1 || n_target > C - 1) return fail(VL_ERR_ARG, "n_target must be 1 .. C - 1");
    k_apgd_targets(logits, labels, B, C, n_target, targets, clean_correct, (hipStream_t)stream);
    return VL_OK;
}

int vl_apgd_step(float* x_adv, float* x_old, float* x_best, float* x_best_adv, float* grad_best, const float* x0,
                 const float* grad, const uint32_t* flags, const float* step, int batch, int64_t image_elems, float eps,
                 float a, int last, void* stream) {
    if (!x_adv || !x_old || !x_best || !x_best_adv || !grad_best || !x0 || !grad || !flags || !step || batch <= 0 || batch > 65535 ||
        image_elems <= 0 || image_elems % 4)
        return fail(VL_ERR_ARG, "bad argument (image_elems must be a positive multiple of 4, batch 1 .. 65535)");
    const void* ptrs[] = {x_adv, x_old, x_best, x_best_adv, grad_best, x0, grad};
    for (const void* p : ptrs)
        if ((uintptr_t)p & 15) return fail(VL_ERR_ARG, "image pointers must be 16-byte aligned");
    k_apgd_step(x_adv, x_old, x_best, x_best_adv, grad_best, x0, grad, flags, step, batch, image_elems, eps, nullptr, nullptr, 0, a,
                last ? 1 : 0, (hipStream_t)stream);
    return VL_OK;
}

int vl_square_step(float* x_cur, float* x_best, const float* x0, const uint32_t* flags, const int32_t* win_prev,
                   const int32_t* win_next, int batch, int image_size, float eps, void* stream) {
    if (!x_cur || !x_best || !x0 || !flags || !win_prev || !win_next || batch <= 0 || batch > 65535 || image_size <= 0 ||
        image_size > 8192)
        return fail(VL_ERR_ARG, "bad argument (batch 1 .. 65535, image_size 1 .. 8192)");
    if (!(eps >= 0.f) || !(eps < INFINITY)) return fail(VL_ERR_ARG, "eps must be finite and >= 0");
    k_square_step(x_cur, x_best, x0, flags, win_prev, win_next, batch, image_size, eps, nullptr, 0, (hipStream_t)stream);
    return VL_OK;
}

// ---- utilities ---------------------------------------------------------------------------------
int vl_channel_affine(float* dst, const float* src, const float scale[3], const float shift[3], int batch, int64_t hw,
                      void* stream) {
    if (!dst || !src || !scale || !shift || batch <= 0 || hw <= 0) return fail(VL_ERR_ARG, "bad argument");
    k_channel_affine(dst, src, scale, shift, batch, hw, (hipStream_t)stream);
    return VL_OK;
}

int vl_adam_step(float* param, const float* grad, float* m1, float* m2, float lr, float b1, float b2, float eps, int t,
                 int64_t n, void* stream) {
    if (!param || !grad || !m1 || !m2 || n <= 0 || t <= 0) return fail(VL_ERR_ARG, "bad argument");
    int* err = nullptr;
    for (const VlFlatRecord& mm : g_vl_models)      // optimizer.step() on a model's flat parameters: its operands are stale now
        if (param < mm.flat + mm.flat_n && param + n > mm.flat) { *mm.dirty = 1; err = *mm.err_flag; }
    k_adam(param, grad, m1, m2, lr, b1, b2, eps, t, n, (hipStream_t)stream, err);
    return VL_OK;
}

int vl_quantize_u8(const float* images, uint8_t* out_hwc, int batch, int channels, int height, int width, void* stream) {
    if (!images || !out_hwc) return fail(VL_ERR_ARG, "null argument");
    k_quantize(images, out_hwc, batch, channels, height, width, (hipStream_t)stream);
    return VL_OK;
}

// ---- profiling -------------------------------------------------------------------------------
int vl_profile_begin(void) {
    if (g_prof) return fail(VL_ERR_STATE, "profile already active");
    g_prof = new Profiler();
    return VL_OK;
}

// Synchronises the device, aggregates per kernel name and writes one JSON object:
// {"name": {"n": launches, "ms": total_ms, "flops": total, "bytes": total, "exec_flops": total}, ...}
// flops / bytes are ALGORITHMIC; exec_flops are the FLOPs the launches issue to the matrix pipes (padded rows,
// padded attention tiles, the whole LoRA K tile) -- bench.py's roofline.path.executed_frac
int vl_profile_report(char* buf, size_t cap) {
    if (!g_prof) return fail(VL_ERR_STATE, "profile not active");
    Profiler* p = g_prof;
    g_prof = nullptr;
    if (hipDeviceSynchronize() != hipSuccess) { delete p; return fail(VL_ERR_HIP, "hipDeviceSynchronize failed"); }
    struct Agg { std::string name; int n; double ms, flops, bytes, exec; };
    std::vector<Agg> agg;
    for (ProfRecord& r : p->recs) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.e0, r.e1);
        (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
        Agg* a = nullptr;
        for (Agg& x : agg) if (x.name == r.name) { a = &x; break; }
        if (!a) { agg.push_back({r.name, 0, 0, 0, 0, 0}); a = &agg.back(); }
        a->n++; a->ms += ms; a->flops += r.flops; a->bytes += r.bytes; a->exec += r.exec_flops;
    }
    delete p;
    std::string out = "{";
    for (size_t i = 0; i < agg.size(); ++i) {
        char line[320];
        snprintf(line, sizeof line, "%s\"%s\": {\"n\": %d, \"ms\": %.6f, \"flops\": %.6e, \"bytes\": %.6e, \"exec_flops\": %.6e}",
                 i ? ", " : "", agg[i].name.c_str(), agg[i].n, agg[i].ms, agg[i].flops, agg[i].bytes, agg[i].exec);
        out += line;
    }
    out += "}";
    if (!buf || cap < out.size() + 1) return fail(VL_ERR_ARG, "buffer too small (%zu needed)", out.size() + 1);
    memcpy(buf, out.c_str(), out.size() + 1);
    return VL_OK;
}

}  // extern "C"
