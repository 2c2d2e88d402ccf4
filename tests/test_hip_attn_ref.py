"""Every attention kernel against a float64 reference, element by element (tests/attn_ref.py states the operands, the reference
and the derived criteria).  vl_debug_attention hands caller-owned buffers to ONE named kernel; no process-wide switch is read.

Conventions: every output lives inside a larger buffer pre-filled with a sentinel (NaN for fp32, a fixed non-grid pattern for
16 bit) with guard rows before and after the result; the guards must survive, and every element of the result is compared (an
element the kernel did not write still holds the sentinel and fails its criterion -- include/vitlora.h: no kernel leaves an
element of its result rows alone).  Each launch runs under the library's profiler, which must have recorded the named kernel and
nothing else.  Structured operands (uniform, permutation) are bit-exact or within the fp32 ulps of 1/l and log2f; continuous and
peaked operands are held to the derived per-element bound.

Token counts: every kernel sees every T it supports -- 2, the multiples of 32 (the unmasked last tile), 33 (<7> with one key in its
second tile), 193 .. 224 (all seven tiles), 200 / 201 (the ring kernel's limit) -- and both instantiations (<1> for T <= 32).
"""
import ctypes as C
import functools
import importlib
import json

import pytest
import torch

import attn_ref as A
import gemm_ref as G
from helpers import PKG, pkg

pytestmark = pytest.mark.gpu

VL_ERR_ARG, VL_ERR_UNSUPPORTED = -1, -4
T_SMALL = [2, 17, 31, 32, 33]
T_FULL = T_SMALL + [63, 64, 65, 160, 192, 193, 197, 199, 200, 201, 223, 224]
T_CLS = T_FULL + [225, 256]
T_PEAKED = [33, 65, 197, 224]
T_DOWN = [17, 33, 197, 200]
GUARD = 4                 # guard rows before and after every output
RATIOS = {}

# name -> (profiler name, direction, family, largest T)
KERNELS = {
    "fwd": ("attn_fwd32_kernel", "fwd", "full", 224), "bwd": ("attn_bwd32_kernel", "bwd", "full", 224),
    "img_fwd": ("attn_fwd_img_kernel", "fwd", "img", 224), "img_bwd": ("attn_bwd_img_kernel", "bwd", "img", 224),
    "ring_bwd": ("attn_bwd_ring_kernel", "bwd", "img", 200),
    "cls_fwd": ("attn_cls_fwd_kernel", "fwd", "cls", 256), "cls_bwd": ("attn_cls_bwd_kernel", "bwd", "cls", 256),
    "f32_mfma_fwd": ("attn_fwd_f32_mfma_kernel", "fwd", "full", 224), "f32_mfma_bwd": ("attn_bwd_f32_mfma_kernel", "bwd", "full", 224),
    "f32_scalar_fwd": ("attn_fwd_f32_kernel", "fwd", "full", 224), "f32_scalar_bwd": ("attn_bwd_f32_kernel", "bwd", "full", 224),
}
K16 = ["fwd", "bwd", "img_fwd", "img_bwd", "ring_bwd", "cls_fwd", "cls_bwd"]
K32 = ["f32_mfma_fwd", "f32_mfma_bwd", "f32_scalar_fwd", "f32_scalar_bwd"]


def t_list(kname):
    fam, tmax = KERNELS[kname][2], KERNELS[kname][3]
    return [t for t in (T_CLS if fam == "cls" else T_FULL) if t <= tmax]


class Ctx:
    def __init__(self, prec):
        P = pkg()
        self.prec = prec
        self.eng = P.Engine(P.ArchConfig(image_size=32, patch_size=16, hidden=128, layers=1, heads=2, mlp=128, num_labels=4),
                            None, precision=prec)
        self.lib, self.h = self.eng.lib, self.eng.h
        self.dtype = A.DTYPES[prec]
        L = importlib.import_module(PKG + "._lib")
        self.CaseT, self.ids = L.VLAttnCase, L.ATTN_KERNELS

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module", params=["f16", "bf16"])
def ctx(request):
    c = Ctx(request.param)
    yield c
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def ctx32():
    c = Ctx("f32")
    yield c
    torch.cuda.synchronize()


# ---- buffers ----------------------------------------------------------------------------------------------------------------
def guarded(rows, cols, dtype):
    """(whole buffer, view of the result rows): sentinel everywhere, GUARD rows before and after the result."""
    if dtype == torch.float32:
        full = torch.full((rows + 2 * GUARD, cols), float("nan"), dtype=dtype, device="cuda")
    else:
        full = torch.full((rows + 2 * GUARD, cols), G.SENTINEL16, dtype=torch.int16, device="cuda").view(dtype)
    return full, full[GUARD:GUARD + rows]


def untouched(buf):
    return torch.isnan(buf) if buf.dtype == torch.float32 else buf.view(torch.int16) == G.SENTINEL16


def guards_intact(full, rows):
    u = untouched(full)
    return bool(u[:GUARD].all()) and bool(u[GUARD + rows:].all())


def sync():
    """Wait for the launch; a device error ends the whole session (nothing more is started on a GPU that reported one)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, session stopped: {e}", returncode=3)


def note_ratio(kernel, prec, criterion, ratio):
    key = (kernel, prec, criterion)
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"RATIO {kernel} {prec} {criterion}: {ratio:.4f} (largest this session {RATIOS[key]:.4f})")


def profiled(ctx, fn):
    """Kernel names (as the library's profiler records them) of the launches fn() makes."""
    assert ctx.lib.vl_profile_begin() == 0
    try:
        fn()
    finally:
        buf = C.create_string_buffer(1 << 16)
        assert ctx.lib.vl_profile_report(buf, len(buf)) == 0
    return set(json.loads(buf.value.decode()))


# ---- cases ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make(kind, B, T, H, prec, cls=False, r=0, mods=0):
    """Operands + float64 reference, computed once and shared by every kernel that runs the case."""
    c = A.BUILDERS[kind](B, T, H, prec, seed=T, cls=cls, r=r, mods=mods)
    return c, A.reference(c, prec)


@functools.lru_cache(maxsize=None)
def criteria(kind, B, T, H, prec, cls, r, mods, direction):
    c, ref = make(kind, B, T, H, prec, cls, r, mods)
    return A.expectations(c, ref, prec, direction)


def launch(ctx, kname, c, ctx_in=None, lse_in=None, down=False):
    """Upload, run the named kernel under the profiler, read back.  Returns the CPU outputs of the result rows."""
    prof_name, direction, fam, _ = KERNELS[kname]
    dt = ctx.dtype
    B, T, H, D = c.B, c.T, c.H, c.D
    cls = fam == "cls"
    crow = B if cls else B * T
    cs = ctx.CaseT()
    cs.B, cs.T, cs.H, cs.kernel = B, T, H, ctx.ids[kname]
    qkv = c.qkv.to(dt).cuda().contiguous()
    cs.qkv = qkv.data_ptr()
    keep, outs = [qkv], {}
    if direction == "fwd":
        cfull, cview = guarded(crow, D, dt)
        lfull, lview = guarded(1, B * H * (1 if cls else T), torch.float32)
        cs.ctx, cs.lse = cview.data_ptr(), lview.data_ptr()
        outs = {"ctx": (cfull, cview, crow), "lse": (lfull, lview, 1)}
    else:
        ci, li = ctx_in.to(dt).cuda().contiguous(), lse_in.float().cuda().contiguous()
        dO = c.dO.to(dt).cuda().contiguous()
        dfull, dview = guarded(B * T, 3 * D, dt)
        keep += [ci, li, dO]
        cs.ctx, cs.lse, cs.dctx, cs.dqkv = ci.data_ptr(), li.data_ptr(), dO.data_ptr(), dview.data_ptr()
        outs = {"dqkv": (dfull, dview, B * T)}
    if down:
        W = (c.Ad if direction == "fwd" else c.Bd).to(dt).cuda().contiguous()
        keep.append(W)
        tfull, tview = guarded(B * T, 64, dt)
        cs.down_W, cs.down_out, cs.r, cs.mods = W.data_ptr(), tview.data_ptr(), c.r, c.mods
        outs["t" if direction == "fwd" else "u"] = (tfull, tview, B * T)
    rc = []

    def go():
        rc.append(ctx.lib.vl_debug_attention(ctx.h, C.byref(cs), ctx.stream()))
        sync()
    names = profiled(ctx, go)
    assert rc == [0], (rc, ctx.lib.vl_last_error())
    assert names == {prof_name}, f"{kname}: the profiler saw {names}"
    got = {}
    for name, (full, view, nrows) in outs.items():
        assert guards_intact(full, nrows), f"{kname} {name}: a guard row was overwritten"
        got[name] = view.cpu()
    if "lse" in got:
        got["lse"] = got["lse"].reshape(B * H, -1)
    if "dqkv" in got:
        d = got.pop("dqkv")
        got["dq"], got["dk"], got["dv"] = (d[:, i * D:(i + 1) * D].contiguous() for i in range(3))
    return got


def check(ctx, kname, c, got, exp, what):
    fails, ratios = A.verify(c, got, exp, ctx.prec)
    for (name, crit), ratio in ratios.items():
        note_ratio(kname, ctx.prec, f"{crit}:{name}", ratio)
    assert not fails, (kname, what, ctx.prec, fails)


def run_case(ctx, kname, kind, B, T, H, r=0, mods=0):
    _, direction, fam, _ = KERNELS[kname]
    cls = fam == "cls"
    c, ref = make(kind, B, T, H, ctx.prec, cls, r, mods)
    exp = criteria(kind, B, T, H, ctx.prec, cls, r, mods, direction)
    ci, li = A.backward_inputs(c, ref, ctx.prec) if direction == "bwd" else (None, None)
    got = launch(ctx, kname, c, ci, li, down=bool(r))
    check(ctx, kname, c, got, exp, (kind, B, T, H, r, mods))


def shapes(T, i):
    """(B, H) of the structured cases at the i-th token count: B * H = 9, 3, 3 (a partly filled block of four waves in the CLS
    kernels; several workgroups in the per-image ones), and the single (image, head) at the smallest counts."""
    return [(3, 3), [(1, 3), (3, 1)][i % 2]] + ([(1, 1)] if T in (2, 17, 33) else [])


def structured(ctx, kname, T):
    i = T_CLS.index(T)
    for B, H in shapes(T, i):
        run_case(ctx, kname, "permutation", B, T, H)
        run_case(ctx, kname, "uniform", B, T, H)


# ---- the 16-bit kernels -----------------------------------------------------------------------------------------------------
SMALL = [(k, t) for k in K16 for t in T_SMALL]
LARGE = [(k, t) for k in K16 for t in t_list(k) if t not in T_SMALL]


@pytest.mark.parametrize("kname,T", SMALL, ids=[f"{k}-{t}" for k, t in SMALL])
def test_structured_small_token_counts(ctx, kname, T):
    """T = 2, 17, 31, 32 (instantiation <1>; 32 takes the unmasked branch) and 33 (<7>: one full tile and one key)."""
    structured(ctx, kname, T)


@pytest.mark.parametrize("kname,T", LARGE, ids=[f"{k}-{t}" for k, t in LARGE])
def test_structured_every_other_token_count(ctx, kname, T):
    structured(ctx, kname, T)


ALL16 = [(k, t) for k in K16 for t in t_list(k)]


@pytest.mark.parametrize("kname,T", ALL16, ids=[f"{k}-{t}" for k, t in ALL16])
def test_continuous_every_token_count(ctx, kname, T):
    run_case(ctx, kname, "continuous", 3, T, 3)
    if T in T_PEAKED:
        run_case(ctx, kname, "peaked_growing", 1, T, 3)
        run_case(ctx, kname, "peaked_first", 3, T, 1)


DOWN_FWD = [(r, t) for r in (4, 8) for t in T_DOWN]
DOWN_BWD = [(k, r, m, t) for k in ("img_bwd", "ring_bwd") for r in (4, 8) for m in (1, 2, 5, 7) for t in T_DOWN]


@pytest.mark.parametrize("r,T", DOWN_FWD, ids=[f"r{r}-{t}" for r, t in DOWN_FWD])
def test_forward_down_projection(ctx, r, T):
    """t = ctx Ad^T inside the per-image forward: exact on the permutation operands, bounded on continuous ones; all 64 columns
    of every token row are written (zeros from column r on)."""
    run_case(ctx, "img_fwd", "permutation", 3, T, 3, r=r, mods=1)
    run_case(ctx, "img_fwd", "continuous", 3, T, 3, r=r, mods=1)


@pytest.mark.parametrize("kname,r,mods,T", DOWN_BWD, ids=[f"{k}-r{r}-m{m}-{t}" for k, r, m, t in DOWN_BWD])
def test_backward_down_projection(ctx, kname, r, mods, T):
    """u = dqkv Bd^T inside both per-image backward kernels: the modules of `mods` at their column groups 0, r, 2r, zeros elsewhere."""
    run_case(ctx, kname, "permutation", 3, T, 3, r=r, mods=mods)
    run_case(ctx, kname, "continuous", 3, T, 3, r=r, mods=mods)


@pytest.mark.parametrize("kname", ["img_fwd", "img_bwd", "ring_bwd"])
@pytest.mark.parametrize("r", [1, 2, 3, 5, 6, 7])
def test_down_projection_ranks_that_are_no_multiple_of_four(ctx, kname, r):
    """The model accepts every rank up to 8 on this path.  The kernels store t / u as 4-element groups at column md * r, so for
    these ranks the groups of neighbouring modules overlap (the later store must win) and the stores are not 8-byte aligned."""
    for T in (17, 33):
        run_case(ctx, kname, "permutation", 3, T, 3, r=r, mods=7)
    run_case(ctx, kname, "continuous", 3, 33, 3, r=r, mods=5 if r % 2 else 7)


@pytest.mark.parametrize("kname,T", [("img_fwd", 2), ("img_bwd", 2), ("ring_bwd", 2), ("img_fwd", 224), ("img_bwd", 224), ("ring_bwd", 192)])
def test_down_projection_at_the_smallest_and_largest_token_counts(ctx, kname, T):
    """T = 224 / 192: every key tile full (the unmasked last tile) together with the down projection; T = 2: one partly filled tile."""
    run_case(ctx, kname, "permutation", 3, T, 3, r=8, mods=7)
    run_case(ctx, kname, "continuous", 3, T, 3, r=4, mods=7)


CHAINS16 = [("fwd", "bwd", 0), ("img_fwd", "img_bwd", 8), ("img_fwd", "ring_bwd", 8), ("cls_fwd", "cls_bwd", 0)]


def chained(ctx, kf, kb, r, T, B=3, H=3):
    """The backward kernel is fed the forward kernel's OWN ctx and lse; its criteria charge the forward's bounds for them."""
    cls = KERNELS[kf][2] == "cls"
    c, ref = make("continuous", B, T, H, ctx.prec, cls, r, 7 if r else 0)
    efwd = criteria("continuous", B, T, H, ctx.prec, cls, r, 7 if r else 0, "fwd")
    gf = launch(ctx, kf, c, down=bool(r))
    check(ctx, kf, c, gf, efwd, ("chain-fwd", T))
    ebwd = A.expectations(c, ref, ctx.prec, "bwd", chained={"ctx": efwd["ctx"][1], "lse": efwd["lse"][1]})
    gb = launch(ctx, kb, c, gf["ctx"], gf["lse"], down=bool(r))
    check(ctx, kb, c, gb, ebwd, ("chain-bwd", T))


@pytest.mark.parametrize("kf,kb,r", CHAINS16, ids=[f"{a}-{b}" for a, b, _ in CHAINS16])
@pytest.mark.parametrize("T", [33, 197])
def test_chained_forward_backward(ctx, kf, kb, r, T):
    chained(ctx, kf, kb, r, T)


# ---- the fp32 kernels -------------------------------------------------------------------------------------------------------
ALL32 = [(k, t) for k in K32 for t in t_list(k)]


@pytest.mark.parametrize("kname,T", ALL32, ids=[f"{k}-{t}" for k, t in ALL32])
def test_f32_kernels_every_token_count(ctx32, kname, T):
    """Permutation operands are exact here too (P = 1 and 0 in fp32); the others are held to the fp32 form of the bound."""
    i = T_CLS.index(T)
    B, H = shapes(T, i)[1]
    run_case(ctx32, kname, "permutation", B, T, H)
    run_case(ctx32, kname, "uniform", B, T, H)
    run_case(ctx32, kname, "continuous", 3, T, 3)
    if T in T_PEAKED:
        run_case(ctx32, kname, "peaked_growing", 1, T, 3)
        run_case(ctx32, kname, "peaked_first", 3, T, 1)


@pytest.mark.parametrize("kf,kb", [("f32_mfma_fwd", "f32_mfma_bwd"), ("f32_scalar_fwd", "f32_scalar_bwd")])
def test_f32_chained_forward_backward(ctx32, kf, kb):
    chained(ctx32, kf, kb, 0, 197)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def refused(ctx, kname, code, B=1, T=17, H=1, mutate=None, down=False, r=4, mods=7):
    """The entry returns `code`, launches nothing and writes nothing."""
    dt = ctx.dtype
    D = 64 * max(H, 1)
    n = max(B, 1) * max(T, 1)
    cs = ctx.CaseT()
    cs.B, cs.T, cs.H, cs.kernel = B, T, H, ctx.ids.get(kname, 99) if isinstance(kname, str) else kname
    bufs = {"qkv": guarded(n, 3 * D, dt), "ctx": guarded(n, D, dt), "lse": guarded(1, n * max(H, 1), torch.float32),
            "dctx": guarded(n, D, dt), "dqkv": guarded(n, 3 * D, dt)}
    for name, (_, view) in bufs.items():
        setattr(cs, name, view.data_ptr())
    if down:
        bufs["down_W"], bufs["down_out"] = guarded(24, 3 * D, dt), guarded(n, 64, dt)
        cs.down_W, cs.down_out, cs.r, cs.mods = bufs["down_W"][1].data_ptr(), bufs["down_out"][1].data_ptr(), r, mods
    if mutate:
        mutate(cs)
    rc = []
    names = profiled(ctx, lambda: (rc.append(ctx.lib.vl_debug_attention(ctx.h, C.byref(cs), ctx.stream())), sync()))
    assert rc == [code], (kname, rc, ctx.lib.vl_last_error())
    assert names == set(), names
    for name, (full, _) in bufs.items():
        assert bool(untouched(full).all()), f"a refused call wrote to {name}"


def test_token_counts_above_a_kernels_limit_are_refused(ctx):
    for kname in ("fwd", "bwd", "img_fwd", "img_bwd"):
        refused(ctx, kname, VL_ERR_UNSUPPORTED, T=225)
    refused(ctx, "ring_bwd", VL_ERR_UNSUPPORTED, T=201)
    refused(ctx, "ring_bwd", VL_ERR_UNSUPPORTED, T=201, down=True)
    for kname in ("cls_fwd", "cls_bwd"):
        refused(ctx, kname, VL_ERR_UNSUPPORTED, T=257)


def test_f32_token_counts_above_the_limit_are_refused(ctx32):
    for kname in K32:
        refused(ctx32, kname, VL_ERR_UNSUPPORTED, T=225)
    refused(ctx32, "fwd", VL_ERR_ARG)                      # a 16-bit kernel on an fp32 handle
    refused(ctx32, "f32_mfma_fwd", VL_ERR_UNSUPPORTED, down=True)


def test_bad_arguments_are_refused(ctx):
    for kname in ("fwd", "bwd", "cls_fwd", "cls_bwd"):
        refused(ctx, kname, VL_ERR_UNSUPPORTED, down=True)            # no fused down projection in these kernels
    refused(ctx, "f32_mfma_fwd", VL_ERR_ARG)                          # an fp32 kernel on a 16-bit handle
    refused(ctx, 99, VL_ERR_ARG)
    refused(ctx, "fwd", VL_ERR_ARG, T=1)
    refused(ctx, "fwd", VL_ERR_ARG, B=0)
    refused(ctx, "fwd", VL_ERR_ARG, H=0)
    for field in ("qkv", "ctx", "lse"):
        refused(ctx, "img_fwd", VL_ERR_ARG, mutate=lambda cs, f=field: setattr(cs, f, None))
        refused(ctx, "img_fwd", VL_ERR_ARG, mutate=lambda cs, f=field: setattr(cs, f, getattr(cs, f) + 8))
    for field in ("dctx", "dqkv"):
        refused(ctx, "ring_bwd", VL_ERR_ARG, mutate=lambda cs, f=field: setattr(cs, f, None))
        refused(ctx, "ring_bwd", VL_ERR_ARG, mutate=lambda cs, f=field: setattr(cs, f, getattr(cs, f) + 8))
    for kname in ("img_fwd", "img_bwd", "ring_bwd"):
        refused(ctx, kname, VL_ERR_ARG, down=True, r=0)
        refused(ctx, kname, VL_ERR_ARG, down=True, r=9)
        refused(ctx, kname, VL_ERR_ARG, down=True, mutate=lambda cs: setattr(cs, "down_out", None))
        refused(ctx, kname, VL_ERR_ARG, down=True, mutate=lambda cs: setattr(cs, "down_W", cs.down_W + 2))
    for kname in ("img_bwd", "ring_bwd"):
        refused(ctx, kname, VL_ERR_ARG, down=True, mods=0)
        refused(ctx, kname, VL_ERR_ARG, down=True, mods=8)
