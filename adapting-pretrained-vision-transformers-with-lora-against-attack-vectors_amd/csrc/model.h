// Model handle, packed weights and workspace of libvitlora_hip.so, shared by the API files
// (vitlora.hip: 16-bit operand path; vit_attacks.hip: the attacks) and the fp32 parity path (vitlora_f32.hip).
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#include "common.h"
// The handle type exists once per build of the 16-bit path (h16 = _Float16 / __bf16 pointer members): the tag itself is renamed
// (vl_model_f16 / vl_model_bf16) and every h16-typed struct below lives in the build's namespace, so no two translation units
// define one name differently (round-4 ADVICE: one-definition rule).  api_dispatch.cpp sees the opaque ABI type only and reads
// the precision through the vl_config the handle starts with (static_assert below).
#define vl_model VL_API(vl_model)
#include "../../include/vitlora.h"
#include "kernels.h"

enum { LQKV = 0, LO = 1, LFC1 = 2, LFC2 = 3 };
static const uint32_t kTargetBits[6] = {VL_T_Q, VL_T_K, VL_T_V, VL_T_O, VL_T_FC1, VL_T_FC2};

namespace VLNS {

struct Slot {           // one adapted module inside a fused projection
    int target_idx;     // 0..5 (q,k,v,o,fc1,fc2)
    int row_off;        // first output row of the module inside the fused projection
    int out, in;
    int ext_off;        // first column of its r slots inside the K extension
    int64_t a_off, b_off;  // offsets into the flat parameter buffer
};

struct Linear {
    int out = 0, in = 0;
    h16* W = nullptr;     // [out, in]
    h16* WT = nullptr;    // [in, out]
    float* bias = nullptr;
    float* Wf32 = nullptr;   // fp32 master: kept when adapters may be merged into W, and in fp32 mode
    float* Wrun = nullptr;   // fp32 mode: the operand the GEMMs read (= Wf32, or the merged copy W + s B A)
    int kext = 0;
    std::vector<Slot> slots;
    h16* Ad = nullptr;    // [kext, in]   t = x Ad^T
    h16* Bu = nullptr;    // [out, kext]  y += t Bu^T        (scaling folded in)
    h16* Bd = nullptr;    // [kext, out]  u = dy Bd^T
    h16* Au = nullptr;    // [in, kext]   dx += u Au^T       (scaling folded in)
};

struct Layer {
    Linear lin[4];
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
};

struct Workspace {
    char* base = nullptr;
    size_t bytes = 0;
    int max_batch = 0, train = 0;
    int64_t Mpad = 0, Mppad = 0;
    h16* patches;
    std::vector<float*> xs;          // 2L+1 residual-stream snapshots [Mpad, D] (fp32 parity mode)
    std::vector<h16*> xs16;          // the same on the 16-bit path: an h16 residual stream (round 4)
    std::vector<float*> mean, rstd;  // 2L
    std::vector<h16*> h1, h2, a;     // per layer in train mode, shared otherwise
    std::vector<h16*> qkv, ctx, z;
    std::vector<float*> lse;
    std::vector<h16*> t[4];          // LoRA down outputs (per layer in train mode)
    float *xhat, *xf, *rstd_f, *logits, *dlogits, *loss, *loss_img;
    float *gscale, *inv_gscale;      // per-image power-of-two gradient scale of the 16-bit backward (and its inverse)
    float* dres[2];                  // fp32 mode: residual-gradient stream (ping-pong)
    h16 *dres_h;                     // 16-bit path: THE residual-gradient stream, updated in place, A operand of the dgrad GEMMs
    h16 *dh, *dctx, *dqkv, *dz, *u;
    h16* xd;                         // train mode: dropout(x) of the current LoRA branch / dgrad temporary [Mpad, MLP]
    float* wg_slab;                  // train mode: [lora_wgrad_chunks(max rows)][flat LoRA elements] per-chunk copies of the LoRA gradient (lora_grad.hip)
    float* grad_img;                 // [max_batch, 3, S, S] for vl_pgd_attack
    // last layer on CLS rows only (cls_path.hip): compact [Bc = round_up(B, 128), .] buffers, 16-bit operand path
    struct Cls {
        int64_t Bc = 0;
        float *x0, *x1, *x2, *mean, *rstd, *lse;     // residual stream before attention / after attention / after the MLP
        h16 *ctx, *delta, *h2, *a, *z, *t;
        float* dres[2];
        h16 *dres_h, *dh, *dctx, *dz, *u;
    } c;
    // persistent staging of vl_pgd_attack: the captured graph only ever sees these addresses
    float *stage_x0, *stage_adv;
    int64_t* stage_labels;
    // ---- fp32 parity mode (vitlora_f32.hip): every activation fp32 ----
    float* f_patches;
    std::vector<float*> f_h1, f_h2, f_a, f_qkv, f_ctx, f_z;
    std::vector<float*> f_t[4];
    float *f_dh, *f_dctx, *f_dqkv, *f_dz, *f_u, *f_xd, *f_tmp;
};

// One forward / backward chain: its activations and what its last forward left behind.  Every launch sequence takes the pass it
// works on as an argument; nothing reads "the current pass" through the handle.
struct Pass {
    Workspace ws;
    int B = 0, rows = 0;             // images and token rows (B * T) of the last forward; B = 0: the pass holds no forward
    int norm = 0, train = 0, cls_only = 0, have_loss = 0;     // cls_only: that forward ran the last layer on the CLS rows only
};

// Cache of captured attack iterations (vit_attacks.hip).  The key is everything an iteration bakes in besides the handle's options
// (a changed option drops the whole cache: drop_graphs); fields a kind does not use stay 0 / nullptr.  PGD: B, chains, eps, alpha
// (its staging buffers live in the workspace).  APGD: B, steps, eps, rho and the caller's scratch, which its kernels read.
// Square: B, steps (n_queries), eps, scratch.  APGD-T: as APGD (the target row it reads sits at a fixed place in the scratch, so
// one entry serves every target and restart).
enum { GRAPH_PGD = 0, GRAPH_APGD = 1, GRAPH_SQUARE = 2, GRAPH_APGDT = 3 };
struct GraphKey {
    int kind, B, chains, steps; float eps, alpha, rho; const void* scratch;
    bool operator==(const GraphKey& o) const {
        return kind == o.kind && B == o.B && chains == o.chains && steps == o.steps && eps == o.eps && alpha == o.alpha && rho == o.rho &&
               scratch == o.scratch;
    }
};
struct GraphEntry { GraphKey key; hipGraphExec_t exec[2]; };   // exec[1]: the second half-batch chain's iteration (side stream), else nullptr

// Hands out consecutive pieces of one buffer, each rounded up to 256 bytes.  base == nullptr: a size query -- every piece comes
// out null and `off` still counts.
struct Carver {
    char* base; size_t off;
    template <class T> T* take(size_t bytes) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += (size_t)round_up((int64_t)bytes, 256);
        return p;
    }
};

// K10 fused into the patch-gradient epilogue: the pixel gradient never goes to HBM (vl_pgd_attack; vl_pgd_step stays the ABI entry)
struct PgdFuse { float* adv; const float* x0; float eps, alpha; };

}  // namespace VLNS

// what the handle-less entry points (vl_adam_step: process_wide.hip) need to know about a live handle of EITHER build
struct VlFlatRecord { void* model; float* flat; int64_t flat_n; int* dirty; int** err_flag; };
// process-wide state, defined once in process_wide.hip (the profiler and the LDS-poison switch: prof.h)
extern std::vector<VlFlatRecord> g_vl_models;      // live handles of BOTH builds (vl_adam_step finds the model a flat buffer belongs to)
extern long long g_poison_count;

struct vl_model {
    vl_config cfg;
    int D, L, H, MLP, S, P, G, NP, T, C, PK;   // PK = 3*P*P
    int r = 0;
    float scaling = 0.f;
    int f32 = 0;                                // cfg.precision == VL_PREC_F32
    int device = 0;
    // embeddings / head
    h16 *Wpe = nullptr, *WpeT = nullptr;
    float* Wpe_f32 = nullptr;                   // fp32 mode
    float *bpe = nullptr, *cls = nullptr, *pos = nullptr, *lnf_g = nullptr, *lnf_b = nullptr;
    std::vector<VLNS::Layer> layers;
    std::vector<void*> allocs;
    // flat trainable parameters: [layer][target]{A,B} ..., classifier W, classifier b
    float* flat = nullptr;
    int64_t flat_n = 0, cls_w_off = 0, cls_b_off = 0;
    int dirty = 1;                              // flat parameters changed since the last vl_lora_commit
    VLNS::Pass main;                            // the whole-batch pass: every API call without chains, the gathered logits / loss with them
    uint64_t drop_seed = 0x5eed, drop_base = 0x5eed, drop_calls = 0;   // LoRA dropout: seed of the last train-mode forward
    // the one cache of captured attack iterations (PGD, APGD, Square: GraphKey above), oldest first, at most 8 (vit_attacks.hip)
    std::vector<VLNS::GraphEntry> graphs;
    hipStream_t cap_stream = nullptr;
    // vl_pgd_attack at small batches (round 4): the batch runs as TWO independent half-batch chains, captured as parallel branches
    // of the one graph (fork / join by events on cap_stream / side_stream) -- a GEMM launch costs about one round more than its
    // tiles (pipeline fill + exposed epilogue), and one chain's ends then meet the other's main loops.  Each chain is a pass of
    // its own (half[c]: workspace carved behind the main one for batches up to CHAIN_MAX_BATCH / 2, and its own forward state).
    static constexpr int CHAIN_MAX_BATCH = 191;     // below the batch at which the per-image attention kernels take over (3/4 of 256 CUs): both forms of a batch then use the same kernels
    VLNS::Pass half[2];
    int chain_batch = 0;          // images each half pass's workspace holds (0: none planned)
    int pgd_chains = 0;           // "pgd_chains" / VITLORA_PGD_CHAINS: 0 = by batch size (2 for 2 <= batch <= 191), 1 = never, 2 = whenever it fits
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // the same two chains behind vl_forward(train = 0) / vl_backward_input (opt-in, "api_chains": the adversarial-patch EoT step runs
    // through these calls): logits are gathered into the main pass, vl_loss_ce works on the whole batch, the backward splits again
    int api_chains = 0;
    int fwd_chains = 0;           // how the last vl_forward ran (0: one chain, the main pass; 2: the two half passes)
    int64_t n_captures = 0, n_commits = 0;
    int use_graph = 1;
    int resid_epi = 2;    // residual add of the 16-bit stream in the GEMM epilogue (EPI_RESID_H16): 1 = attention output projection, 2 = + fc2, 0 = LayerNorm-side
    int plan_batch = 0, plan_train = 0;
    int attn_img_mode = -1;   // VITLORA_ATTN_IMG: 1 / 0 force the per-image attention kernels on / off, -1 = by batch size
    int num_cus = 256;
    int dead_rows = 1;        // eval-mode forward / backward: last layer on CLS rows only (VITLORA_DEAD_ROWS=0 or vl_debug_set_dead_rows: off)
    int fuse_down_min_k = 2048;   // LoRA down projection inside the ping-pong GEMM for projections at least this deep (VITLORA_FUSE_DOWN_MIN_K)
    int small_m_rows = 16384;     // token rows up to which the "small batch" forms apply (VITLORA_SMALL_M_ROWS; batch <= 83 at T = 197)
    int fuse_pgd = 1;         // vl_pgd_attack: PGD step inside the patch-gradient epilogue (VITLORA_FUSE_PGD=0: separate K10 launch)
    int square_bare = 0;      // "square_bare" = 1: the Square replay is the forward alone (timing baseline of tools/square_bench.py)
    int* err_flag = nullptr;                    // pinned host word written by kernels (bad label, ...), read at API entry
    float mean[3] = {0.485f, 0.456f, 0.406f};   // get_normalization, Utils.py:92-93
    float stdv[3] = {0.229f, 0.224f, 0.225f};
};

static_assert(offsetof(vl_model, cfg) == 0, "api_dispatch.cpp reads the precision through the vl_config the handle starts with");

int vl_fail(int code, const char* fmt, ...);      // process_wide.hip: records the text vl_last_error returns, returns `code`
#define HIPCHK(expr)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return vl_fail(VL_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
// helpers defined in vitlora.hip
namespace VLNS {
bool capturing(hipStream_t s);            // the stream is inside a stream capture (launch errors are then read after the replay)
bool vl_drop_on(const vl_model* m, const Pass& p);      // LoRA dropout applies to the forward that pass `p` holds
int check_async(vl_model* m);             // errors a kernel reported through the pinned host word, surfaced by the next API call
int check_launch(const char* what);       // sticky launch failures, read after a launch sequence that ran OUTSIDE stream capture
int chain_resources(vl_model* m);         // side stream and fork / join events of the two half-batch chains, created on first use
// one forward of B images in pass `p`; on success p holds it (B, rows, norm, train, cls_only) and no loss yet
int forward_impl(vl_model* m, Pass& p, const float* x, int B, int normalise, int train, hipStream_t s);
// shared dgrad chain: flat_grad != null additionally produces the LoRA / classifier gradients, grad_x != null the input gradient,
// pf != null applies the PGD step in the patch-gradient epilogue instead
int backward_impl(vl_model* m, Pass& p, float* grad_x, float* flat_grad, hipStream_t s, const PgdFuse* pf = nullptr);

// runs fn(c, half pass c, its stream) for both half passes -- chain 0 on `s`, chain 1 on the side stream -- between the fork and
// the join event; returns the first failure
template <typename F>
int on_both_halves(vl_model* m, hipStream_t s, F fn) {
    HIPCHK(hipEventRecord(m->ev_fork, s));
    HIPCHK(hipStreamWaitEvent(m->side_stream, m->ev_fork, 0));
    const int rc0 = fn(0, m->half[0], s), rc1 = fn(1, m->half[1], m->side_stream);
    HIPCHK(hipEventRecord(m->ev_join, m->side_stream));
    HIPCHK(hipStreamWaitEvent(s, m->ev_join, 0));
    return rc0 ? rc0 : rc1;
}

// graph cache, defined in vit_attacks.hip
void drop_graphs(vl_model* m);            // destroys every cached iteration (an option or the workspace changed; vl_destroy)

// fp32 parity path (vitlora_f32.hip): reached through the fp16 build only (vl_create_bf16 refuses VL_PREC_F32)
#ifdef VL_BF16
static inline size_t f32_carve(const vl_model*, Workspace&, int, Carver& cv) { return cv.off; }
static inline int f32_forward(vl_model*, Pass&, const float*, int, int, hipStream_t) { return VL_ERR_STATE; }
static inline int f32_backward(vl_model*, Pass&, float*, float*, hipStream_t) { return VL_ERR_STATE; }
static inline int f32_init(int) { return 0; }
static inline int f32_debug_gemm(const vl_gemm_case*, hipStream_t) { return VL_ERR_STATE; }
static inline int f32_debug_attention(const vl_attn_case*, hipStream_t) { return VL_ERR_STATE; }
#else
size_t f32_carve(const vl_model* m, Workspace& w, int train, Carver& cv);      // goes on from cv; w.Mpad / w.Mppad are set by the caller
int f32_forward(vl_model* m, Pass& p, const float* x, int B, int normalise, hipStream_t s);  // p.train / p.rows are set by the caller
int f32_backward(vl_model* m, Pass& p, float* grad_x, float* flat_grad, hipStream_t s);
int f32_init(int device);     // kernel attributes; 0 = ok
int f32_debug_gemm(const vl_gemm_case* c, hipStream_t s);   // vl_debug_gemm on an fp32 handle: validates, then one k_gemm_f32
int f32_debug_attention(const vl_attn_case* c, hipStream_t s);   // vl_debug_attention on an fp32 handle (validated by the caller): one fp32 attention kernel
#endif
}  // namespace VLNS
