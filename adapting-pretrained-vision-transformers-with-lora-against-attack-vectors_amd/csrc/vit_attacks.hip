// The attacks on the ViT handle (include/vitlora.h): PGD, Auto-PGD (APGD-CE, APGD-T) and Square, each a device-resident loop whose one
// iteration is captured once as a hipGraph and replayed.  This file holds the ONE cache of those graphs (GraphKey / GraphEntry:
// model.h), the one capture sequence, the one rule for "eager or replay", the attacks' scratch layouts and their entry points.
// Forward, backward and the workspace are vitlora.hip's (helpers declared in model.h); all arithmetic is in the kernel files.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.h"
#include "api_rename.h"     // handle-taking entry points are declared and defined as vl_*_f16 / vl_*_bf16 (api_dispatch.cpp exports the ABI names)
#include "model.h"
#include "prof.h"

#define fail vl_fail

namespace VLNS {

namespace {

// VITLORA_GRAPH_DUMP: a file path, nullptr when unset or empty (the third switch that is neither a flag nor an integer: vitlora.hip)
const char* env_graph_dump() { const char* e = getenv("VITLORA_GRAPH_DUMP"); return e && e[0] ? e : nullptr; }

// VITLORA_GRAPH_DUMP=<file>: append the node list of a captured iteration (type, kernel name, grid, block, dynamic LDS)
void dump_graph(hipGraph_t graph) {
    const char* path = env_graph_dump();
    if (!path) return;
    FILE* f = fopen(path, "a");
    if (!f) return;
    size_t n = 0;
    if (hipGraphGetNodes(graph, nullptr, &n) != hipSuccess) { fclose(f); return; }
    std::vector<hipGraphNode_t> nodes(n);
    if (n && hipGraphGetNodes(graph, nodes.data(), &n) != hipSuccess) { fclose(f); return; }
    fprintf(f, "graph %zu nodes\n", n);
    for (size_t i = 0; i < n; ++i) {
        hipGraphNodeType ty;
        if (hipGraphNodeGetType(nodes[i], &ty) != hipSuccess) { fprintf(f, "%zu ?\n", i); continue; }
        if (ty == hipGraphNodeTypeKernel) {
            hipKernelNodeParams kp;
            memset(&kp, 0, sizeof kp);
            if (hipGraphKernelNodeGetParams(nodes[i], &kp) != hipSuccess) { fprintf(f, "%zu kernel ?\n", i); continue; }
            const char* nm = hipKernelNameRefByPtr(kp.func, nullptr);
            fprintf(f, "%zu kernel %s grid %u,%u,%u block %u lds %u\n", i, nm ? nm : "?", kp.gridDim.x, kp.gridDim.y, kp.gridDim.z,
                    kp.blockDim.x, kp.sharedMemBytes);
        } else if (ty == hipGraphNodeTypeMemset) {
            hipMemsetParams mp;
            memset(&mp, 0, sizeof mp);
            if (hipGraphMemsetNodeGetParams(nodes[i], &mp) != hipSuccess) { fprintf(f, "%zu memset ?\n", i); continue; }
            fprintf(f, "%zu memset dst %p value %u elem %u width %zu height %zu\n", i, mp.dst, mp.value, mp.elementSize, mp.width, mp.height);
        } else {
            fprintf(f, "%zu type %d\n", i, (int)ty);
        }
    }
    {   // dependency edges as index pairs
        size_t ne = 0;
        if (hipGraphGetEdges(graph, nullptr, nullptr, &ne) == hipSuccess && ne) {
            std::vector<hipGraphNode_t> from(ne), to(ne);
            if (hipGraphGetEdges(graph, from.data(), to.data(), &ne) == hipSuccess) {
                auto idx = [&](hipGraphNode_t x) -> long { for (size_t i = 0; i < n; ++i) if (nodes[i] == x) return (long)i; return -1; };
                fprintf(f, "edges %zu:", ne);
                for (size_t e = 0; e < ne; ++e) fprintf(f, " %ld>%ld", idx(from[e]), idx(to[e]));
                fprintf(f, "\n");
            }
        } else fprintf(f, "edges 0\n");
    }
    (void)hipGetLastError();
    fclose(f);
}

// ---- the graph cache ---------------------------------------------------------------------------
void destroy_entry(GraphEntry& e) {
    for (hipGraphExec_t& x : e.exec)
        if (x) { (void)hipGraphExecDestroy(x); x = nullptr; }
}

// Captures what fn(stream) enqueues and instantiates it.  Captured cold: nothing has to run eagerly first.  (Round 2 ran the first
// iteration eagerly because replays of a graph captured in a fresh process differed from the eager result.  Cause, established in
// round 3 with tools/cold_capture_diag.py: the two hipMemsetAsync nodes of the backward did not take effect on replays when they
// were captured before the runtime's fill kernel had ever run; the first launch passed only because the workspace was still zero.
// They are k_zero kernel nodes now: profiles/r03_cold_capture_*.txt.)  The capture runs on a private stream (the caller's may be
// the legacy default stream, which cannot capture); nothing executes during capture, the graph is launched on the caller's stream.
template <typename F>
int capture_graph(vl_model* m, F fn, hipGraphExec_t* out) {
    if (!m->cap_stream) HIPCHK(hipStreamCreateWithFlags(&m->cap_stream, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    (void)hipGetLastError();
    HIPCHK(hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = fn(m->cap_stream);
    hipError_t e = hipStreamEndCapture(m->cap_stream, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return fail(VL_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    dump_graph(graph);
    e = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(VL_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
    return VL_OK;
}

// The cached entry of `key`; on a miss fn(c, stream) is captured for each of the key's chains -- one graph per chain, each over its
// own activation workspace -- and the entry joins the cache, which holds the 8 most recent ones (first in, first out).
template <typename F>
int cached_graphs(vl_model* m, const GraphKey& key, F fn, const GraphEntry** out) {
    for (const GraphEntry& g : m->graphs)
        if (g.key == key) { *out = &g; return VL_OK; }
    GraphEntry e = {key, {nullptr, nullptr}};
    for (int c = 0; c < key.chains; ++c)
        if (const int rc = capture_graph(m, [&](hipStream_t s) { return fn(c, s); }, &e.exec[c])) { destroy_entry(e); return rc; }
    if (m->graphs.size() >= 8) { destroy_entry(m->graphs.front()); m->graphs.erase(m->graphs.begin()); }
    m->graphs.push_back(e);
    m->n_captures++;
    *out = &m->graphs.back();
    return VL_OK;
}

// `count` iterations of an attack on `s`; fn(c, stream) enqueues one iteration of chain c.  Eager when the handle does not use
// graphs, under the profiler and under the LDS poison hook (both work per launch); otherwise the key's graphs are replayed.
// Two chains (vl_pgd_attack): chain 1 runs on the side stream -- eagerly between a fork and a join event per iteration, replayed as
// a graph of its own beside chain 0's, the two streams meeting only at the start and the end of the attack.
template <typename F>
int run_iterations(vl_model* m, const char* who, const GraphKey& key, int count, hipStream_t s, F fn) {
    const bool two = key.chains == 2;
    if (!m->use_graph || g_prof || g_poison_lds) {
        for (int i = 0; i < count; ++i)
            if (const int rc = two ? on_both_halves(m, s, [&](int c, Pass&, hipStream_t sc) { return fn(c, sc); }) : fn(0, s)) return rc;
        return check_launch(who);
    }
    const GraphEntry* g = nullptr;
    if (const int rc = cached_graphs(m, key, fn, &g)) return rc;
    if (two) {
        HIPCHK(hipEventRecord(m->ev_fork, s));
        HIPCHK(hipStreamWaitEvent(m->side_stream, m->ev_fork, 0));
    }
    for (int i = 0; i < count; ++i) {
        HIPCHK(hipGraphLaunch(g->exec[0], s));
        if (two) HIPCHK(hipGraphLaunch(g->exec[1], m->side_stream));
    }
    if (two) {
        HIPCHK(hipEventRecord(m->ev_join, m->side_stream));
        HIPCHK(hipStreamWaitEvent(s, m->ev_join, 0));
    }
    return VL_OK;
}

// ---- caller-owned scratch of APGD and Square ---------------------------------------------------
struct ScratchSpec {        // the nouns of one attack's messages and its size function
    const char *attack, *count, *size_fn;
    size_t (*bytes)(const vl_model* m, int batch, int n);
};
int check_attack_scratch(const vl_model* m, const ScratchSpec& k, const void* scratch, size_t bytes, int batch, int n) {
    if (!m->main.ws.max_batch) return fail(VL_ERR_STATE, "no workspace");
    if (batch <= 0 || batch > m->main.ws.max_batch) return fail(VL_ERR_STATE, "batch exceeds planned workspace");
    if (batch > 65535) return fail(VL_ERR_UNSUPPORTED, "%s runs at most 65535 images per call (one grid row per image)", k.attack);
    if (n < 1 || n > 65535) return fail(VL_ERR_ARG, "%s must be 1 .. 65535", k.count);
    if (!scratch || ((uintptr_t)scratch & 255)) return fail(VL_ERR_ARG, "scratch must be a 256-byte aligned device buffer");
    const size_t need = k.bytes(m, batch, n);
    if (bytes < need) return fail(VL_ERR_ARG, "%s scratch too small: %zu < %zu (%s)", k.attack, bytes, need, k.size_fn);
    return VL_OK;
}

// ---- PGD ---------------------------------------------------------------------------------------
int pgd_iteration(vl_model* m, Pass& p, const float* x0, const int64_t* labels, int B, float eps, float alpha, float* adv, hipStream_t s) {
    int rc = forward_impl(m, p, adv, B, 1, 0, s);
    if (rc) return rc;
    k_ce_loss(p.ws.logits, labels, B, m->C, p.ws.dlogits, p.ws.loss_img, p.ws.loss, m->err_flag, s);
    p.have_loss = 1;
    if (m->fuse_pgd && !m->f32) {
        const PgdFuse pf = {adv, x0, eps, alpha};
        return backward_impl(m, p, nullptr, nullptr, s, &pf);
    }
    rc = backward_impl(m, p, p.ws.grad_img, nullptr, s);
    if (rc) return rc;
    k_pgd_step(adv, x0, p.ws.grad_img, eps, alpha, 0.f, 1.f, (int64_t)B * 3 * m->S * m->S, s, m->err_flag);
    return VL_OK;
}

// ---- Auto-PGD (APGD-CE, L-inf; include/vitlora.h) -----------------------
// Everything the attack keeps between iterations, carved from the caller's scratch (base == nullptr: size only).
struct ApgdLayout {
    float *x0, *x_adv, *x_old, *x_best, *x_best_adv, *grad_best;
    int64_t* labels;
    ApgdState st;
};
size_t apgd_carve(const vl_model* m, int B, int N, char* base, ApgdLayout& L) {
    Carver cv{base, 0};
    const size_t img = (size_t)B * 3 * m->S * m->S * 4, row = (size_t)B * 4;
    L.x0 = cv.take<float>(img); L.x_adv = cv.take<float>(img); L.x_old = cv.take<float>(img);
    L.x_best = cv.take<float>(img); L.x_best_adv = cv.take<float>(img); L.grad_best = cv.take<float>(img);
    L.labels = cv.take<int64_t>((size_t)B * 8);
    L.st.ctr = cv.take<int32_t>(16);
    L.st.sched = cv.take<ApgdSched>((size_t)(N + 1) * sizeof(ApgdSched));
    L.st.step = cv.take<float>(row); L.st.loss_best = cv.take<float>(row); L.st.loss_best_last = cv.take<float>(row);
    L.st.reduced_last = cv.take<int32_t>(row); L.st.robust = cv.take<int32_t>(row); L.st.flags = cv.take<uint32_t>(row);
    L.st.tr_loss = cv.take<float>((size_t)(N + 1) * row); L.st.tr_step = cv.take<float>((size_t)N * row);
    L.st.tr_pred = cv.take<int32_t>((size_t)(N + 1) * row);
    return cv.off;
}
size_t apgd_bytes(const vl_model* m, int batch, int steps) { ApgdLayout sz; return apgd_carve(m, batch, steps, nullptr, sz); }
const ScratchSpec kApgdScratch = {"APGD", "steps", "vl_apgd_scratch_bytes", apgd_bytes};

// one APGD / APGD-T iteration in the main pass: evaluate x_adv (forward, the loss that loss(p, s) launches -- CE or DLR-targeted --,
// gradient to grad_img), then bookkeeping and the next point
template <typename LossFn>
int apgd_iteration(vl_model* m, const ApgdLayout& L, int B, int N, float eps, float rho, hipStream_t s, LossFn loss) {
    Pass& p = m->main;
    int rc = forward_impl(m, p, L.x_adv, B, 1, 0, s);
    if (rc) return rc;
    loss(p, s);
    p.have_loss = 1;
    if ((rc = backward_impl(m, p, p.ws.grad_img, nullptr, s))) return rc;
    k_apgd_track(L.st, p.ws.loss_img, p.ws.logits, L.labels, B, m->C, N, eps, rho, s);
    k_apgd_step(L.x_adv, L.x_old, L.x_best, L.x_best_adv, L.grad_best, L.x0, p.ws.grad_img, L.st.flags, L.st.step, B,
                (int64_t)3 * m->S * m->S, eps, L.st.sched, L.st.ctr, N, 0.f, 0, s, m->err_flag);
    return VL_OK;
}

// ---- APGD-T (targeted Auto-PGD on the DLR loss, L-inf; include/vitlora.h) ----
// APGD's layout first (so target_cur, which the captured iteration reads, sits at a place that does not depend on the number of
// targets), then the fold's state and the target table.
struct ApgdtLayout {
    ApgdLayout a;
    int32_t *target_cur, *still[2], *clean_correct, *fooled_by, *targets;
    float* x_out;
};
size_t apgdt_carve(const vl_model* m, int B, int N, int n_target, char* base, ApgdtLayout& L) {
    Carver cv{base, apgd_carve(m, B, N, base, L.a)};
    const size_t img = (size_t)B * 3 * m->S * m->S * 4, row = (size_t)B * 4;
    L.target_cur = cv.take<int32_t>(row);
    L.still[0] = cv.take<int32_t>(row); L.still[1] = cv.take<int32_t>(row);
    L.clean_correct = cv.take<int32_t>(row); L.fooled_by = cv.take<int32_t>(row);
    L.x_out = cv.take<float>(img);
    L.targets = cv.take<int32_t>((size_t)n_target * row);
    return cv.off;
}
// the shared scratch check sizes APGD's part (batch, steps); the whole size is checked by the caller, which knows n_target
size_t apgdt_bytes_min(const vl_model* m, int batch, int steps) { ApgdtLayout sz; return apgdt_carve(m, batch, steps, 1, nullptr, sz); }
const ScratchSpec kApgdtScratch = {"APGD-T", "steps", "vl_apgdt_scratch_bytes", apgdt_bytes_min};

// ---- Square attack (L-inf, margin loss; include/vitlora.h) -------------
// Everything the attack keeps between replays, carved from the caller's scratch (base == nullptr: size only).
struct SquareLayout {
    float *x0, *x_cur, *x_best;
    int64_t* labels;
    SquareState st;
};
size_t square_carve(const vl_model* m, int B, int N, char* base, SquareLayout& L) {
    Carver cv{base, 0};
    const size_t img = (size_t)B * 3 * m->S * m->S * 4, row = (size_t)B * 4;
    L.x0 = cv.take<float>(img); L.x_cur = cv.take<float>(img); L.x_best = cv.take<float>(img);
    L.labels = cv.take<int64_t>((size_t)B * 8);
    L.st.ctr = cv.take<int32_t>(16);
    L.st.par = cv.take<SquareParams>(sizeof(SquareParams));
    L.st.side = cv.take<int32_t>((size_t)(N + 1) * 4);
    L.st.margin_min = cv.take<float>(row); L.st.queries = cv.take<int32_t>(row); L.st.robust = cv.take<int32_t>(row);
    L.st.flags = cv.take<uint32_t>(row);
    L.st.win_prev = cv.take<int32_t>(4 * row); L.st.win_next = cv.take<int32_t>(4 * row);
    L.st.tr_margin = cv.take<float>((size_t)(N + 1) * row);
    L.st.tr_win = cv.take<int32_t>((size_t)N * 4 * row);
    return cv.off;
}
size_t square_bytes(const vl_model* m, int batch, int n_queries) { SquareLayout sz; return square_carve(m, batch, n_queries, nullptr, sz); }
const ScratchSpec kSquareScratch = {"Square", "n_queries", "vl_square_scratch_bytes", square_bytes};
int square_check_scratch(const vl_model* m, const void* scratch, size_t bytes, int batch, int n_queries) {
    if (m->C < 2) return fail(VL_ERR_UNSUPPORTED, "the margin loss needs num_labels >= 2");
    return check_attack_scratch(m, kSquareScratch, scratch, bytes, batch, n_queries);
}

// one replay in the main pass: evaluate x_cur (eval-mode forward, the last layer on the CLS rows alone), then the bookkeeping and
// the pixels of the two windows
int square_iteration(vl_model* m, const SquareLayout& L, int B, int N, float eps, hipStream_t s) {
    Pass& p = m->main;
    const int rc = forward_impl(m, p, L.x_cur, B, 1, 0, s);
    if (rc) return rc;
    if (m->square_bare) return VL_OK;
    k_square_track(L.st, p.ws.logits, L.labels, B, m->C, m->S, N, s, m->err_flag);
    k_square_step(L.x_cur, L.x_best, L.x0, L.st.flags, L.st.win_prev, L.st.win_next, B, m->S, eps, L.st.ctr, N, s);
    return VL_OK;
}

}  // namespace

void drop_graphs(vl_model* m) {
    for (GraphEntry& g : m->graphs) destroy_entry(g);
    m->graphs.clear();
}

extern "C" {

int vl_pgd_attack(vl_model* m, const float* x0, const int64_t* labels, int batch, float eps, float alpha, int steps,
                  int random_start, uint64_t seed, float* adv_out, void* stream) {
    if (!m || !x0 || !labels || !adv_out) return fail(VL_ERR_ARG, "bad argument");
    if (!m->main.ws.max_batch) return fail(VL_ERR_STATE, "no workspace");
    if (batch <= 0 || batch > m->main.ws.max_batch) return fail(VL_ERR_STATE, "batch exceeds planned workspace");
    hipStream_t s = (hipStream_t)stream;
    int rc = check_async(m);
    if (rc) return rc;
    if (m->dirty && (rc = vl_lora_commit(m, stream))) return rc;     // the attack sees the CURRENT adapters
    Workspace& w = m->main.ws;
    const int64_t n = (int64_t)batch * 3 * m->S * m->S;
    // Persistent staging: the captured iteration only ever reads / writes the workspace's x0 / labels / adv buffers,
    // so ONE cache entry per (batch, eps, alpha, chains) serves every batch of a run whatever tensors the caller passes
    // (3 device copies of the image batch per attack: < 0.1 % of a PGD-20 attack).
    HIPCHK(hipMemcpyAsync(w.stage_x0, x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(w.stage_labels, labels, (size_t)batch * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    if (random_start) k_pgd_init(w.stage_adv, w.stage_x0, eps, 0.f, 1.f, seed, n, s);
    else HIPCHK(hipMemcpyAsync(w.stage_adv, w.stage_x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    // two half-batch chains, each a pass of its own over its slice of the staged batch (model.h): by batch size, or as "pgd_chains" says
    const int b0 = (batch + 1) / 2, b1 = batch - b0;
    const bool chain_fits = m->chain_batch > 0 && batch >= 2 && b0 <= m->chain_batch;
    const int chains = (chain_fits && (m->pgd_chains == 2 || (m->pgd_chains == 0 && batch <= vl_model::CHAIN_MAX_BATCH))) ? 2 : 1;
    const int64_t off1 = (int64_t)b0 * 3 * m->S * m->S;
    // one PGD iteration of chain c: the whole batch in the main pass, or half pass c over its slice
    auto iteration = [&](int c, hipStream_t sc) -> int {
        if (chains == 1) return pgd_iteration(m, m->main, w.stage_x0, w.stage_labels, batch, eps, alpha, w.stage_adv, sc);
        return pgd_iteration(m, m->half[c], w.stage_x0 + (c ? off1 : 0), w.stage_labels + (c ? b0 : 0), c ? b1 : b0, eps, alpha,
                             w.stage_adv + (c ? off1 : 0), sc);
    };
    m->fwd_chains = 0;
    if (chains == 2 && (rc = chain_resources(m))) return rc;
    if (steps > 0) {
        const GraphKey key = {GRAPH_PGD, batch, chains, 0, eps, alpha, 0.f, nullptr};
        if ((rc = run_iterations(m, "vl_pgd_attack", key, steps, s, iteration))) return rc;
        // two chains leave no forward of the whole batch in the main pass: a backward call needs its own forward and loss
        if (chains == 2) m->main.B = m->main.have_loss = 0;
    }
    HIPCHK(hipMemcpyAsync(adv_out, w.stage_adv, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return VL_OK;
}

int vl_apgd_scratch_bytes(vl_model* m, int batch, int steps, size_t* bytes) {
    if (!m || !bytes || batch <= 0 || steps < 1 || steps > 65535) return fail(VL_ERR_ARG, "bad argument");
    *bytes = apgd_bytes(m, batch, steps);
    return VL_OK;
}

int vl_apgd_attack(vl_model* m, const vl_apgd_args* a) {
    if (!m || !a || !a->x0 || !a->labels) return fail(VL_ERR_ARG, "bad argument");
    if (!(a->eps >= 0.f) || !(a->eps < INFINITY) || !(a->rho >= 0.f) || !(a->rho <= 1.f)) return fail(VL_ERR_ARG, "eps must be finite and >= 0, rho in [0, 1]");
    int rc = check_attack_scratch(m, kApgdScratch, a->scratch, a->scratch_bytes, a->batch, a->steps);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)a->stream;
    if ((rc = check_async(m))) return rc;
    if (m->dirty && (rc = vl_lora_commit(m, a->stream))) return rc;     // the attack sees the CURRENT adapters
    const int B = a->batch, N = a->steps;
    const float eps = a->eps, rho = a->rho;
    ApgdLayout L;
    apgd_carve(m, B, N, (char*)a->scratch, L);
    const int64_t n_img = (int64_t)3 * m->S * m->S, n = (int64_t)B * n_img;
    // staging, as vl_pgd_attack: the captured iteration only ever sees addresses inside the scratch and the workspace
    HIPCHK(hipMemcpyAsync(L.x0, a->x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(L.labels, a->labels, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    if (a->x_init) k_apgd_start(L.x_adv, a->x_init, n, s);
    else if (a->random_start) k_apgd_rand_init(L.x_adv, L.x0, eps, a->seed, B, n_img, s);
    else k_apgd_start(L.x_adv, L.x0, n, s);
    HIPCHK(hipMemcpyAsync(L.x_old, L.x_adv, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    k_apgd_sched(L.st.sched, L.st.ctr, N, s);
    m->fwd_chains = 0;
    const GraphKey key = {GRAPH_APGD, B, 1, N, eps, 0.f, rho, a->scratch};
    auto ce_loss = [&](Pass& p, hipStream_t sc) {
        k_ce_loss(p.ws.logits, L.labels, B, m->C, p.ws.dlogits, p.ws.loss_img, p.ws.loss, m->err_flag, sc);
    };
    if ((rc = run_iterations(m, "vl_apgd_attack", key, N + 1, s, [&](int, hipStream_t sc) { return apgd_iteration(m, L, B, N, eps, rho, sc, ce_loss); })))
        return rc;
    const size_t row = (size_t)B * 4;
    if (a->x_best) HIPCHK(hipMemcpyAsync(a->x_best, L.x_best, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (a->x_best_adv) HIPCHK(hipMemcpyAsync(a->x_best_adv, L.x_best_adv, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (a->loss_best) HIPCHK(hipMemcpyAsync(a->loss_best, L.st.loss_best, row, hipMemcpyDeviceToDevice, s));
    if (a->robust) HIPCHK(hipMemcpyAsync(a->robust, L.st.robust, row, hipMemcpyDeviceToDevice, s));
    if (a->trace_loss) HIPCHK(hipMemcpyAsync(a->trace_loss, L.st.tr_loss, (size_t)(N + 1) * row, hipMemcpyDeviceToDevice, s));
    if (a->trace_step) HIPCHK(hipMemcpyAsync(a->trace_step, L.st.tr_step, (size_t)N * row, hipMemcpyDeviceToDevice, s));
    if (a->trace_pred) HIPCHK(hipMemcpyAsync(a->trace_pred, L.st.tr_pred, (size_t)(N + 1) * row, hipMemcpyDeviceToDevice, s));
    return VL_OK;
}

int vl_debug_apgd_track(vl_model* m, const vl_apgd_track_case* c, void* stream) {
    if (!m || !c || !c->loss_img || !c->logits || !c->labels) return fail(VL_ERR_ARG, "bad argument");
    int rc = check_attack_scratch(m, kApgdScratch, c->scratch, c->scratch_bytes, c->batch, c->steps);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ApgdLayout L;
    apgd_carve(m, c->batch, c->steps, (char*)c->scratch, L);
    if (c->reset) k_apgd_sched(L.st.sched, L.st.ctr, c->steps, s);
    k_apgd_track(L.st, c->loss_img, c->logits, c->labels, c->batch, m->C, c->steps, c->eps, c->rho, s);
    HIPCHK(hipMemcpyAsync(L.st.ctr, L.st.ctr + 1, 4, hipMemcpyDeviceToDevice, s));      // what the step kernel does in the attack
    const size_t row = (size_t)c->batch * 4;
    if (c->step_out) HIPCHK(hipMemcpyAsync(c->step_out, L.st.step, row, hipMemcpyDeviceToDevice, s));
    if (c->flags_out) HIPCHK(hipMemcpyAsync(c->flags_out, L.st.flags, row, hipMemcpyDeviceToDevice, s));
    if (c->loss_best_out) HIPCHK(hipMemcpyAsync(c->loss_best_out, L.st.loss_best, row, hipMemcpyDeviceToDevice, s));
    if (c->robust_out) HIPCHK(hipMemcpyAsync(c->robust_out, L.st.robust, row, hipMemcpyDeviceToDevice, s));
    return VL_OK;
}

int vl_apgdt_scratch_bytes(vl_model* m, int batch, int steps, int n_target_classes, size_t* bytes) {
    if (!m || !bytes || batch <= 0 || steps < 1 || steps > 65535 || n_target_classes < 1 || n_target_classes > 65535)
        return fail(VL_ERR_ARG, "bad argument");
    ApgdtLayout sz;
    *bytes = apgdt_carve(m, batch, steps, n_target_classes, nullptr, sz);
    return VL_OK;
}

int vl_apgdt_attack(vl_model* m, const vl_apgdt_args* a) {
    if (!m || !a || !a->x0 || !a->labels) return fail(VL_ERR_ARG, "bad argument");
    if (m->C < 4) return fail(VL_ERR_UNSUPPORTED, "the DLR loss needs num_labels >= 4");
    if (a->n_target_classes < 1 || a->n_target_classes > m->C - 1) return fail(VL_ERR_ARG, "n_target_classes must be 1 .. num_labels - 1");
    if (a->n_restarts < 1) return fail(VL_ERR_ARG, "n_restarts must be >= 1");
    if (!(a->eps >= 0.f) || !(a->eps < INFINITY) || !(a->rho >= 0.f) || !(a->rho <= 1.f)) return fail(VL_ERR_ARG, "eps must be finite and >= 0, rho in [0, 1]");
    int rc = check_attack_scratch(m, kApgdtScratch, a->scratch, a->scratch_bytes, a->batch, a->steps);
    if (rc) return rc;
    const int B = a->batch, N = a->steps, K = a->n_target_classes, R = a->n_restarts;
    ApgdtLayout L;
    const size_t need = apgdt_carve(m, B, N, K, (char*)a->scratch, L);
    if (a->scratch_bytes < need) return fail(VL_ERR_ARG, "APGD-T scratch too small: %zu < %zu (vl_apgdt_scratch_bytes)", a->scratch_bytes, need);
    hipStream_t s = (hipStream_t)a->stream;
    if ((rc = check_async(m))) return rc;
    if (m->dirty && (rc = vl_lora_commit(m, a->stream))) return rc;     // the attack sees the CURRENT adapters
    const float eps = a->eps, rho = a->rho;
    const int64_t n_img = (int64_t)3 * m->S * m->S, n = (int64_t)B * n_img;
    const size_t row = (size_t)B * 4;
    // staging, as vl_apgd_attack: the captured iteration only ever sees addresses inside the scratch and the workspace
    HIPCHK(hipMemcpyAsync(L.a.x0, a->x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(L.a.labels, a->labels, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(L.x_out, L.a.x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    // the clean pass: clean_correct and the target table
    m->fwd_chains = 0;
    if ((rc = forward_impl(m, m->main, L.a.x0, B, 1, 0, s))) return rc;
    k_apgd_targets(m->main.ws.logits, L.a.labels, B, m->C, K, L.targets, L.clean_correct, s);
    if (a->targets_in) HIPCHK(hipMemcpyAsync(L.targets, a->targets_in, (size_t)K * row, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(L.still[0], L.clean_correct, row, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemsetAsync(L.fooled_by, 0xFF, row, s));                  // -1
    const GraphKey key = {GRAPH_APGDT, B, 1, N, eps, 0.f, rho, a->scratch};
    auto dlr_loss = [&](Pass& p, hipStream_t sc) {      // APGD's iteration with the DLR-targeted loss towards target_cur
        k_dlr_targeted_loss(p.ws.logits, L.a.labels, L.target_cur, B, m->C, p.ws.dlogits, p.ws.loss_img, p.ws.loss, m->err_flag, sc);
    };
    int run = 0;
    for (int k = 0; k < K; ++k) {
        HIPCHK(hipMemcpyAsync(L.target_cur, L.targets + (size_t)k * B, row, hipMemcpyDeviceToDevice, s));
        for (int r = 0; r < R; ++r, ++run) {
            k_apgd_rand_init(L.a.x_adv, L.a.x0, eps, a->seed + (uint64_t)run, B, n_img, s);
            HIPCHK(hipMemcpyAsync(L.a.x_old, L.a.x_adv, n * sizeof(float), hipMemcpyDeviceToDevice, s));
            k_apgd_sched(L.a.st.sched, L.a.st.ctr, N, s);
            if ((rc = run_iterations(m, "vl_apgdt_attack", key, N + 1, s, [&](int, hipStream_t sc) { return apgd_iteration(m, L.a, B, N, eps, rho, sc, dlr_loss); })))
                return rc;
            if (a->loss_best) HIPCHK(hipMemcpyAsync(a->loss_best + (size_t)run * B, L.a.st.loss_best, row, hipMemcpyDeviceToDevice, s));
            if (a->robust_run) HIPCHK(hipMemcpyAsync(a->robust_run + (size_t)run * B, L.a.st.robust, row, hipMemcpyDeviceToDevice, s));
            k_apgdt_fold(L.x_out, L.a.x_best_adv, L.still[run & 1], L.still[(run + 1) & 1], L.a.st.robust, L.fooled_by, run, B, n_img, s);
        }
    }
    if (a->x_adv) HIPCHK(hipMemcpyAsync(a->x_adv, L.x_out, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (a->robust) HIPCHK(hipMemcpyAsync(a->robust, L.still[run & 1], row, hipMemcpyDeviceToDevice, s));
    if (a->clean_correct) HIPCHK(hipMemcpyAsync(a->clean_correct, L.clean_correct, row, hipMemcpyDeviceToDevice, s));
    if (a->targets) HIPCHK(hipMemcpyAsync(a->targets, L.targets, (size_t)K * row, hipMemcpyDeviceToDevice, s));
    if (a->fooled_by) HIPCHK(hipMemcpyAsync(a->fooled_by, L.fooled_by, row, hipMemcpyDeviceToDevice, s));
    if (a->trace_loss) HIPCHK(hipMemcpyAsync(a->trace_loss, L.a.st.tr_loss, (size_t)(N + 1) * row, hipMemcpyDeviceToDevice, s));
    if (a->trace_step) HIPCHK(hipMemcpyAsync(a->trace_step, L.a.st.tr_step, (size_t)N * row, hipMemcpyDeviceToDevice, s));
    if (a->trace_pred) HIPCHK(hipMemcpyAsync(a->trace_pred, L.a.st.tr_pred, (size_t)(N + 1) * row, hipMemcpyDeviceToDevice, s));
    return VL_OK;
}

int vl_square_scratch_bytes(vl_model* m, int batch, int n_queries, size_t* bytes) {
    if (!m || !bytes || batch <= 0 || n_queries < 1 || n_queries > 65535) return fail(VL_ERR_ARG, "bad argument");
    *bytes = square_bytes(m, batch, n_queries);
    return VL_OK;
}

int vl_square_attack(vl_model* m, const vl_square_args* a) {
    if (!m || !a) return fail(VL_ERR_ARG, "bad argument");
    if (a->first < 0 || a->count < 1) return fail(VL_ERR_ARG, "first must be >= 0 and count >= 1");
    if (a->first == 0 && (!a->x0 || !a->labels)) return fail(VL_ERR_ARG, "x0 and labels are needed when first == 0");
    if (!(a->eps >= 0.f) || !(a->eps < INFINITY) || !(a->p_init > 0.f) || !(a->p_init <= 1.f))
        return fail(VL_ERR_ARG, "eps must be finite and >= 0, p_init in (0, 1]");
    int rc = square_check_scratch(m, a->scratch, a->scratch_bytes, a->batch, a->n_queries);
    if (rc) return rc;
    if ((int64_t)a->first + a->count > (int64_t)a->n_queries + 1) return fail(VL_ERR_ARG, "first + count exceeds the n_queries + 1 replays of the schedule");
    hipStream_t s = (hipStream_t)a->stream;
    if ((rc = check_async(m))) return rc;
    if (m->dirty && (rc = vl_lora_commit(m, a->stream))) return rc;     // the attack sees the CURRENT adapters
    const int B = a->batch, N = a->n_queries;
    const float eps = a->eps;
    SquareLayout L;
    square_carve(m, B, N, (char*)a->scratch, L);
    const int64_t n = (int64_t)B * 3 * m->S * m->S;
    if (a->first == 0) {
        // staging, as vl_pgd_attack: the captured iteration only ever sees addresses inside the scratch and the workspace
        HIPCHK(hipMemcpyAsync(L.x0, a->x0, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(L.labels, a->labels, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        SquareSched sc;
        square_schedule(m->S, N, a->p_init, &sc);
        k_square_sched(L.st, sc, N, a->seed, a->image_offset, s);
        k_square_init(L.x_cur, L.x_best, L.x0, L.st.par, B, m->S, eps, s);
    }
    m->fwd_chains = 0;
    const GraphKey key = {GRAPH_SQUARE, B, 1, N, eps, 0.f, 0.f, a->scratch};
    if ((rc = run_iterations(m, "vl_square_attack", key, a->count, s, [&](int, hipStream_t sc) { return square_iteration(m, L, B, N, eps, sc); })))
        return rc;
    const size_t row = (size_t)B * 4;
    const int done = a->first + a->count;          // replays 0 .. done - 1 have run
    if (a->x_best) HIPCHK(hipMemcpyAsync(a->x_best, L.x_best, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (a->margin_min) HIPCHK(hipMemcpyAsync(a->margin_min, L.st.margin_min, row, hipMemcpyDeviceToDevice, s));
    if (a->queries) HIPCHK(hipMemcpyAsync(a->queries, L.st.queries, row, hipMemcpyDeviceToDevice, s));
    if (a->robust) HIPCHK(hipMemcpyAsync(a->robust, L.st.robust, row, hipMemcpyDeviceToDevice, s));
    if (a->trace_margin) HIPCHK(hipMemcpyAsync(a->trace_margin, L.st.tr_margin, (size_t)done * row, hipMemcpyDeviceToDevice, s));
    if (a->trace_win) HIPCHK(hipMemcpyAsync(a->trace_win, L.st.tr_win, (size_t)std::min(done, N) * 4 * row, hipMemcpyDeviceToDevice, s));
    return VL_OK;
}

int vl_debug_square_track(vl_model* m, const vl_square_track_case* c, void* stream) {
    if (!m || !c || !c->logits || !c->labels) return fail(VL_ERR_ARG, "bad argument");
    if (c->reset && (!(c->p_init > 0.f) || !(c->p_init <= 1.f))) return fail(VL_ERR_ARG, "p_init in (0, 1]");
    int rc = square_check_scratch(m, c->scratch, c->scratch_bytes, c->batch, c->n_queries);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    SquareLayout L;
    square_carve(m, c->batch, c->n_queries, (char*)c->scratch, L);
    if (c->reset) {
        SquareSched sc;
        square_schedule(m->S, c->n_queries, c->p_init, &sc);
        k_square_sched(L.st, sc, c->n_queries, c->seed, c->image_offset, s);
    }
    k_square_track(L.st, c->logits, c->labels, c->batch, m->C, m->S, c->n_queries, s, nullptr);
    HIPCHK(hipMemcpyAsync(L.st.ctr, L.st.ctr + 1, 4, hipMemcpyDeviceToDevice, s));      // what the step kernel does in the attack
    const size_t row = (size_t)c->batch * 4;
    if (c->flags_out) HIPCHK(hipMemcpyAsync(c->flags_out, L.st.flags, row, hipMemcpyDeviceToDevice, s));
    if (c->win_prev_out) HIPCHK(hipMemcpyAsync(c->win_prev_out, L.st.win_prev, 4 * row, hipMemcpyDeviceToDevice, s));
    if (c->win_next_out) HIPCHK(hipMemcpyAsync(c->win_next_out, L.st.win_next, 4 * row, hipMemcpyDeviceToDevice, s));
    if (c->margin_min_out) HIPCHK(hipMemcpyAsync(c->margin_min_out, L.st.margin_min, row, hipMemcpyDeviceToDevice, s));
    if (c->queries_out) HIPCHK(hipMemcpyAsync(c->queries_out, L.st.queries, row, hipMemcpyDeviceToDevice, s));
    return VL_OK;
}

}  // extern "C"

}  // namespace VLNS
