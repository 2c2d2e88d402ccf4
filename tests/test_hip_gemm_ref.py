"""Every GEMM kernel and fused epilogue against a float64 reference, element by element (tests/gemm_ref.py states the
operands, the reference and the criteria).  vl_debug_gemm hands caller-owned buffers to ONE chosen kernel:
route 1 = 128-row tile kernel, 2 = persistent 256-row kernel, 3 = ping-pong kernel, 4 = streaming kernel, 0 = launch_gemm's pick.

Conventions: grid operands unless "continuous" is named; every output buffer is larger than the result and pre-filled with a
sentinel (NaN for fp32, a fixed non-grid pattern for 16 bit) that must survive everywhere outside the result -- pad columns
between the width and the pitch, rows past M, rows past Mvalid, columns past n_store; input pad columns hold NaN, so a kernel
that multiplied them would poison its result.  The persistent kernels run with the CU count shrunk (vl_debug_set_cus) so that a
small product still makes each workgroup walk several tiles.

Not reachable here: the 64-row form of the skinny kernel (VITLORA_SKINNY_BM=64 is read once per process at gemm_init; a test
would need a process of its own), so the skinny cases run the default 128-row form only.
"""
import ctypes as C
import functools
import importlib
from contextlib import contextmanager

import pytest
import torch

import gemm_ref as G
from gemm_ref import Case
from helpers import PKG, pkg

pytestmark = pytest.mark.gpu

PRECS = ["f16", "bf16"]
VL_ERR_ARG, VL_ERR_UNSUPPORTED, VL_ERR_NONFINITE = -1, -4, -5
RATIOS = {}            # (kernel, prec, criterion) -> largest error / allowed seen in this session (printed per test)


class Ctx:
    def __init__(self, prec):
        P = pkg()
        self.prec = prec
        self.eng = P.Engine(P.ArchConfig(image_size=32, patch_size=16, hidden=128, layers=1, heads=2, mlp=128, num_labels=4),
                            None, precision=prec)
        self.lib, self.h = self.eng.lib, self.eng.h
        self.dtype = G.DTYPES.get(prec, torch.float32)
        self.dev_cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.CaseT = importlib.import_module(PKG + "._lib").VLGemmCase

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @contextmanager
    def cus(self, n):
        """Persistent-grid size of the 256-row, ping-pong and streaming kernels; the device's count is restored on exit."""
        if n is None:
            yield
            return
        try:
            assert self.lib.vl_debug_set_cus(self.h, n) == 0
            yield
        finally:
            assert self.lib.vl_debug_set_cus(self.h, self.dev_cus) == 0


@pytest.fixture(scope="module", params=PRECS)
def ctx(request):
    c = Ctx(request.param)
    yield c
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def ctx32():
    c = Ctx("f32")
    yield c
    torch.cuda.synchronize()


# ---- device buffers -------------------------------------------------------------------------------------------------------
def dev_in(t, dtype, pitch=None, rows=None):
    """[rows, pitch] device copy of the 2-D CPU tensor t; pad columns / rows hold NaN."""
    r, w = t.shape
    rows, pitch = rows or r, pitch or w
    buf = torch.full((rows, pitch), float("nan"), dtype=dtype, device="cuda")
    buf[:r, :w] = t.to(dtype).cuda()
    return buf


def sentinel_buf(rows, pitch, dtype):
    if dtype == torch.float32:
        return torch.full((rows, pitch), float("nan"), dtype=dtype, device="cuda")
    return torch.full((rows, pitch), G.SENTINEL16, dtype=torch.int16, device="cuda").view(dtype)


def untouched(buf):
    """Boolean map of the elements that still hold the sentinel."""
    if buf.dtype == torch.float32:
        return torch.isnan(buf)
    return buf.view(torch.int16) == G.SENTINEL16


def ptr(t):
    return None if t is None else t.data_ptr()


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
    """Kernel names (as the library's profiler records them) of the launches fn() makes; fn's own return value is checked by fn."""
    import json
    assert ctx.lib.vl_profile_begin() == 0
    try:
        fn()
    finally:
        buf = C.create_string_buffer(1 << 16)
        assert ctx.lib.vl_profile_report(buf, len(buf)) == 0
    return set(json.loads(buf.value.decode()))


ROUTE_NAME = {0: "default", 1: "gemm128", 2: "gemm256", 3: "gemm_pp", 4: "gemm_stream"}


def kernel_name(route, bn, tag=""):
    """Name under which a case's error / allowed ratio is recorded: the skinny 64-column forms are kernels of their own."""
    name = {(1, 64): "skinny64", (0, 64): "skinny64", (4, 64): "gemm_stream64"}.get((route, bn), ROUTE_NAME[route])
    return name + (f"[{tag}]" if tag else "")


# ---- cases ----------------------------------------------------------------------------------------------------------------
def gelu_scale(K):
    """Power of two that keeps z = sum of K grid products (variance 0.14 each) at a standard deviation of about 3: z covers
    [-6, 6]."""
    s = 1.0
    while (K * 0.14) ** 0.5 * s > 4.0:
        s *= 0.5
    return s


@functools.lru_cache(maxsize=None)
def linear_case(epi, M, N, K1, K2, seed=0, kind="grid", prec=None, lora_zero_upper=False, with_G=False, p=0.5, down=0,
                ones_col=False, down_cols=0):
    """Operands + float64 reference of one row-layout case, computed once and shared by every route / CU count that runs it.
    Grid values are the same numbers in fp16 and bf16, so grid cases without a rounded intermediate share one reference
    (prec=None); continuous cases and fused-down cases (t is rounded to the operand type) are per type."""
    gen = torch.Generator().manual_seed(1000 + seed)
    dtype = G.DTYPES[prec] if prec else torch.float64
    K = K1 + K2
    if kind == "grid":
        ws = gelu_scale(K) if epi == "gelu" else 1.0
        A1, W1 = G.grid(gen, (M, K1)), G.grid(gen, (N, K1), scale=ws)
        A2 = G.grid(gen, (M, K2)) if K2 else None
        W2 = G.grid(gen, (N, K2), scale=ws) if K2 else None
        bias = G.grid(gen, (N,))
        R = G.grid(gen, (M, N))
        Gf = G.grid(gen, (M, N)) if with_G else None
    else:
        A1, W1 = G.activations(gen, (M, K1), dtype), G.weights(gen, (N, K1), dtype)
        A2 = G.activations(gen, (M, K2), dtype) if K2 else None
        W2 = G.weights(gen, (N, K2), dtype) if K2 else None
        bias = 0.1 * torch.randn(N, generator=gen)
        R = torch.randn(M, N, generator=gen)
        R = R if epi == "resid_f32" else R.to(dtype)
        Gf = G.activations(gen, (M, N), dtype) if with_G else None
    if lora_zero_upper:
        W2[:, 32:] = 0
    c = Case(epi=epi, A1=A1, W1=W1, A2=A2, W2=W2, bias=bias)
    if epi in ("resid_f32", "resid_h16", "gelu_bwd", "drop_acc"):
        c.R = R
    if epi == "drop_acc":
        c.G, c.drop = Gf, (0x1234 + seed, 7, p)
    if down:
        dw = torch.zeros(64, K1, dtype=torch.float64)
        dw[:down] = G.grid(gen, (down, K1))            # rows of Ad in use, zero padded
        c.down_W, c.down_cols, c.A2, c.ones_col = dw, down_cols or 64, None, ones_col
        if ones_col:
            c.W2 = c.W2.clone()
            c.W2[:, 63] = bias                          # the bias rides in column 63 of the LoRA K tile
            c.bias = None
    ref = G.reference(c, dtype if prec else torch.float16)
    if kind == "grid":
        # products of two k/8 values (GELU cases: W scaled by the power of two ws, the bias a multiple of 1/8 still); with the down
        # projection inside, t (multiples of 1/64 rounded to 11 / 8 bits) times k/8.
        # (the factors of gelu_bwd / drop_acc multiply the FINAL sum once: 18 + 4 bits, exact)
        G.exact_guard(ref["abs_z"], 2.0 ** -9 if down else 2.0 ** -6 * ws)
    return c, ref


def run_linear(ctx, c, ref, *, route, bn=128, n_store=0, k2_used=0, pad=8, tight_ldc=False, cus=None, alias_R=False,
               down_groups=0, want_t=False):
    """Upload, run, read back.  Returns dict of CPU outputs restricted to the result; asserts every sentinel outside it."""
    dt = ctx.dtype
    e = c.epi
    M, N = ref["z"].shape
    K1 = c.A1.shape[1]
    K2 = c.W2.shape[1] if c.W2 is not None else 0
    width = n_store or N
    f32out = e in G.F32_OUT
    odt = torch.float32 if f32out else dt
    ldc = width if tight_ldc else width + pad
    cs = ctx.CaseT()
    cs.M, cs.N, cs.K1, cs.K2, cs.epi, cs.bn, cs.route = M, N, K1, K2, G.EPI[e], bn, route
    cs.n_store, cs.k2_used = n_store, k2_used
    keep = []

    def up(t, dtype, pitch):
        b = dev_in(t, dtype, pitch)
        keep.append(b)
        return b
    a1 = up(c.A1, dt, K1 + pad); cs.A1, cs.lda1 = ptr(a1), K1 + pad
    w1 = up(c.W1, dt, K1 + pad); cs.W1, cs.ldw1 = ptr(w1), K1 + pad
    if K2:
        w2 = up(c.W2, dt, K2 + pad); cs.W2, cs.ldw2 = ptr(w2), K2 + pad
        if c.A2 is not None:
            a2 = up(c.A2, dt, K2 + pad); cs.A2, cs.lda2 = ptr(a2), K2 + pad
    if c.bias is not None:
        b = c.bias.float().cuda(); keep.append(b); cs.bias = ptr(b)
    Cbuf = sentinel_buf(M + 16, ldc, odt)
    cs.C, cs.ldc = ptr(Cbuf), ldc
    C2buf = None
    if e == "gelu":
        C2buf = sentinel_buf(M + 16, ldc, odt)
        cs.C2, cs.ldc2 = ptr(C2buf), ldc
    if c.R is not None:
        if alias_R:                                     # R aliasing C: the accumulate form
            Cbuf[:M, :width] = c.R[:, :width].to(odt).cuda()
            cs.R, cs.ldr = ptr(Cbuf), ldc
        else:
            rdt = torch.float32 if e == "resid_f32" else dt
            r = up(c.R[:, :width], rdt, width + pad); cs.R, cs.ldr = ptr(r), width + pad
    if c.G is not None:
        g = up(c.G[:, :width], dt, width + pad); cs.G, cs.ldg = ptr(g), width + pad
    if e == "drop_acc":
        cs.drop_seed, cs.drop_stream, cs.drop_p = c.drop
    tbuf = None
    if c.down_W is not None:
        dw = up(c.down_W, dt, K1 + pad); cs.down_W, cs.down_ldw = ptr(dw), K1 + pad
        cs.down_groups, cs.ones_col = down_groups or 1, int(c.ones_col)
        if want_t:
            tbuf = sentinel_buf(M + 16, 64 + pad, dt)
            cs.down_out, cs.down_ld = ptr(tbuf), 64 + pad
    with ctx.cus(cus):
        rc = ctx.lib.vl_debug_gemm(ctx.h, C.byref(cs), ctx.stream())
        sync()
    assert rc == 0, (rc, ctx.lib.vl_last_error())
    out = {}
    live = torch.zeros_like(Cbuf, dtype=torch.bool)
    live[:M, :width] = True
    for name, buf in (("C", Cbuf), ("C2", C2buf)):
        if buf is None:
            continue
        assert bool(untouched(buf)[~live].all()), f"{name}: a sentinel outside the {M} x {width} result was overwritten"
        out[name] = buf[:M, :width].cpu()
    if tbuf is not None:
        cols = 16 * cs.down_groups
        tl = torch.zeros_like(tbuf, dtype=torch.bool)
        tl[:M, :cols] = True
        assert bool(untouched(tbuf)[~tl].all()), "t: a sentinel outside its columns was overwritten"
        out["t"] = tbuf[:M, :cols].cpu()
    return out


def check_linear(ctx, c, ref, out, *, route, kind="grid", n_store=0, K=None, bn=128, tag=""):
    """The criterion of gemm_ref's docstring for this epilogue / operand kind."""
    e = c.epi
    kname = kernel_name(route, bn, tag)
    width = n_store or ref["z"].shape[1]
    odt = torch.float32 if e in G.F32_OUT else ctx.dtype
    rC = ref["C"][:, :width]
    if e == "gelu":
        for which, name in ((0, "C"), (1, "C2")):
            r = ref[name][:, :width]
            n, where, ratio = G.compare_bounded(out[name], r, G.gelu_allowed(ref["z"][:, :width], r, which, ctx.dtype))
            note_ratio(kname, ctx.prec, "gelu" if which == 0 else "gelu'", ratio)
            assert n == 0, (name, n, where)
    elif kind == "grid" and not (e == "drop_acc" and c.drop[2] != 0.5):
        n, where = G.compare_exact(out["C"], rC, odt)
        assert n == 0, (n, where)
    else:
        n, where, ratio = G.compare_bounded(out["C"], rC, G.continuous_allowed(rC, ref["abs"][:, :width], K, odt))
        note_ratio(kname, ctx.prec, "continuous", ratio)
        assert n == 0, (n, where)
    if "t" in out:
        n, where = G.compare_exact(out["t"], ref["t"][:, :out["t"].shape[1]], ctx.dtype)
        assert n == 0, ("t", n, where)


ALIAS = {"resid_f32"}      # R aliases C for the fp32 residual form (the accumulate form the library uses)


def go(ctx, epi, M, N, K1, K2, *, route, seed=0, kind="grid", cus=None, **kw):
    prec = ctx.prec if kind != "grid" else None
    case_kw = {k: kw.pop(k) for k in ("lora_zero_upper", "with_G", "p") if k in kw}
    tag = kw.pop("tag", "")
    c, ref = linear_case(epi, M, N, K1, K2, seed, kind, prec, **case_kw)
    out = run_linear(ctx, c, ref, route=route, cus=cus, alias_R=epi in ALIAS, **kw)
    check_linear(ctx, c, ref, out, route=route, kind=kind, n_store=kw.get("n_store", 0), K=K1 + K2, bn=kw.get("bn", 128), tag=tag)


# ---- 128-row kernel -------------------------------------------------------------------------------------------------------
SHAPES128 = [(128, 128, 64, 0), (128, 128, 128, 64), (384, 384, 192, 128)]     # the last: 9 tiles (xcd_remap remainder), two LoRA tiles
LINEAR_EPIS = ["store_h16", "resid_f32", "gelu", "gelu_bwd", "resid_h16", "store_f32"]


@pytest.mark.parametrize("shape", SHAPES128, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("epi", LINEAR_EPIS)
def test_gemm128_every_linear_epilogue(ctx, epi, shape):
    go(ctx, epi, *shape, route=1)


@pytest.mark.parametrize("shape", SHAPES128, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("with_G", [False, True])
def test_gemm128_drop_acc_half_is_bit_exact(ctx, with_G, shape):
    go(ctx, "drop_acc", *shape, route=1, with_G=with_G, p=0.5)


@pytest.mark.parametrize("with_G", [False, True])
def test_gemm128_drop_acc_tenth_continuous(ctx, with_G):
    go(ctx, "drop_acc", 128, 128, 64, 64, route=1, kind="continuous", with_G=with_G, p=0.1)


@pytest.mark.parametrize("n_store", [16, 48])
@pytest.mark.parametrize("epi", ["store_h16", "resid_h16"])
def test_gemm128_narrow_rows(ctx, epi, n_store):
    go(ctx, epi, 128, 128, 128, 64, route=1, n_store=n_store, tight_ldc=True)
    go(ctx, epi, 128, 128, 128, 64, route=0, n_store=n_store, tight_ldc=True)


@pytest.mark.parametrize("epi", ["store_h16", "resid_h16", "store_f32"])
def test_gemm128_continuous(ctx, epi):
    go(ctx, epi, 256, 128, 64, 64, route=1, kind="continuous")


@pytest.mark.parametrize("shape", [(128, 64, 64, 0), (256, 64, 768, 0)], ids=lambda s: "x".join(map(str, s)))
def test_skinny_form(ctx, shape):
    go(ctx, "store_h16", *shape, route=1, bn=64)
    go(ctx, "store_h16", *shape, route=0, bn=64)


def test_skinny_form_continuous(ctx):
    go(ctx, "store_h16", 256, 64, 128, 0, route=1, bn=64, kind="continuous")


# ---- 256-row persistent kernel ----------------------------------------------------------------------------------------------
def gemm256_heights(M, N, cus):
    """Tile heights the launcher of gemm256.hip uses for M x N on `cus` workgroups, restated from its planning rule so that every
    case below NAMES the instantiations it reaches (and fails if the rule moves a case elsewhere): rows are 256-row tiles except a
    tail of 128-row tiles that fits one round; a round of 256-row tiles costs 1, the tail launch 0.55; fewest big rows given up
    wins ties.  On the whole device every shape here fits one round of 128-row tiles: small tiles only."""
    tn, r256, r128 = N // 256, M // 256, M // 128
    best, pick = 1e30, None
    for give in range(r256 + 1):
        nb, ns = (r256 - give) * tn, (r128 - 2 * (r256 - give)) * tn
        if ns > cus:
            break
        cost = -(-nb // cus) + (0.55 if ns else 0.0)
        if cost < best - 1e-9:
            best, pick = cost, (nb, ns)
    return {h for h, n in zip((256, 128), pick) if n}


def go256(ctx, epi, M, N, K1, K2, *, cus, heights=None, **kw):
    """Route 2, with the profiler's kernel names checked against the tile heights the case is meant to reach."""
    want = gemm256_heights(M, N, cus or ctx.dev_cus)
    assert heights is None or want == set(heights), (want, heights)
    names = profiled(ctx, lambda: go(ctx, epi, M, N, K1, K2, route=2, cus=cus, **kw))
    assert names == {f"gemm256_kernel<{h}, {G.EPI[epi]}>" for h in want}, names


# cus3: 128 x N, 256 x 256 and 384 x 256 are small tiles only, 256 x 512 big tiles only, 384 x 512 one big row plus the 128-row tail
# launch, 640 x N two big rows (4 tiles on 3 workgroups at N = 512) plus the tail.  small_only: the device's CU count, where every
# one of these shapes is a single round of 128-row tiles.
@pytest.mark.parametrize("cus", [3, None], ids=["cus3", "small_only"])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("M", [128, 256, 384, 640])
def test_gemm256_tile_walk(ctx, M, N, cus):
    go256(ctx, "store_h16", M, N, 64, 64, cus=cus)


@pytest.mark.parametrize("shape,cus,heights", [((640, 512, 128, 0), 3, (256, 128)), ((384, 256, 64, 64), None, (128,))],
                         ids=["640x512x128_big_and_tail", "384x256x64+64_small_only"])
@pytest.mark.parametrize("epi", LINEAR_EPIS)
def test_gemm256_every_linear_epilogue(ctx, epi, shape, cus, heights):
    go256(ctx, epi, *shape, cus=cus, heights=heights)


@pytest.mark.parametrize("epi", ["store_h16", "resid_h16", "gelu"])
def test_gemm256_deep_k(ctx, epi):
    """4 big tiles walked by 3 workgroups (one of them runs two) and a 128-row tail, 49 K tiles each."""
    go256(ctx, epi, 640, 512, 3072, 64, cus=3, heights=(256, 128))


@pytest.mark.parametrize("k2_used,zero_upper", [(8, True), (24, True), (32, True), (0, False), (40, False)])
def test_gemm256_lora_half_tile_skip(ctx, k2_used, zero_upper):
    """k2_used <= 32 lets the kernel skip the upper half of the LoRA K tile (its W2 columns are zero then); 0 (unknown) and 40
    must not skip: all 64 columns are nonzero.  On both tile heights: 2 big tiles and 2 tail tiles."""
    go256(ctx, "store_h16", 384, 512, 128, 64, cus=3, heights=(256, 128), seed=3 if zero_upper else 4, k2_used=k2_used,
          lora_zero_upper=zero_upper)


@pytest.mark.parametrize("M,cus,heights", [(384, 3, (256, 128)), (256, 3, (256,)), (384, None, (128,))], ids=["big_and_tail", "big", "small"])
@pytest.mark.parametrize("epi", ["store_h16", "store_f32"])
def test_gemm256_continuous(ctx, epi, M, cus, heights):
    go256(ctx, epi, M, 512, 64, 64, cus=cus, heights=heights, kind="continuous", tag="+".join(map(str, heights)))


# ---- ping-pong kernel -----------------------------------------------------------------------------------------------------
# (M, N, CUs): tiles per workgroup 1, 2 (one pair), 3 (pair + single tail), 4, 5; then 9 tiles on 3 workgroups, 8 tiles on 3
PP_WALKS = [(128, 256, 1), (256, 256, 1), (384, 256, 1), (256, 512, 1), (640, 256, 1), (384, 768, 3), (512, 512, 3)]


@pytest.mark.parametrize("M,N,cus", PP_WALKS)
def test_gemm_pp_tile_walk(ctx, M, N, cus):
    go(ctx, "store_h16", M, N, 768, 64, route=3, cus=cus)


@pytest.mark.parametrize("K1,K2", [(768, 0), (768, 64), (832, 0), (832, 64), (3072, 0), (3072, 64)])
@pytest.mark.parametrize("epi", ["store_h16", "gelu", "gelu_bwd", "store_f32", "resid_h16"])
def test_gemm_pp_depths_and_epilogues(ctx, epi, K1, K2):
    go(ctx, epi, 384, 256, K1, K2, route=3, cus=1)


@pytest.mark.parametrize("K1", [768, 3072])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("epi", ["store_h16", "resid_h16"])
def test_gemm_pp_fused_down_projection(ctx, epi, groups, K1):
    """Result AND t against the reference (not against the skinny kernel); resid_h16 takes its bias from column 63 of W2."""
    ones = epi == "resid_h16"
    c, ref = linear_case(epi, 384, 256, K1, 64, 5, "grid", ctx.prec, down=16 * groups - 8, ones_col=ones, down_cols=16 * groups)
    out = run_linear(ctx, c, ref, route=3, cus=1, down_groups=groups, want_t=True)
    check_linear(ctx, c, ref, out, route=3)
    out = run_linear(ctx, c, ref, route=3, cus=3, down_groups=groups, want_t=False)      # down_out is optional
    check_linear(ctx, c, ref, out, route=3)


@pytest.mark.parametrize("epi", ["store_h16", "resid_h16", "store_f32"])
def test_gemm_pp_continuous(ctx, epi):
    go(ctx, epi, 384, 256, 768, 0, route=3, cus=1, kind="continuous")


# ---- streaming kernel (row thresholds bypassed by the forced route) -----------------------------------------------------------
@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("M", [128, 384, 1152])
def test_gemm_stream_ragged_walk(ctx, M, N):
    go(ctx, "store_h16", M, N, 128, 64, route=4, cus=3)


@pytest.mark.parametrize("K1,K2", [(64, 0), (128, 64), (768, 64)])
@pytest.mark.parametrize("epi", ["store_h16", "gelu", "gelu_bwd"])
def test_gemm_stream_depths_and_epilogues(ctx, epi, K1, K2):
    go(ctx, epi, 384, 384, K1, K2, route=4, cus=3)


@pytest.mark.parametrize("shape", [(384, 64, 128, 0), (1152, 64, 64, 0)], ids=lambda s: "x".join(map(str, s)))
def test_gemm_stream_64_column_form(ctx, shape):
    go(ctx, "store_h16", *shape, route=4, bn=64, cus=3)


def test_gemm_stream_narrow_rows(ctx):
    go(ctx, "store_h16", 384, 128, 128, 0, route=4, cus=3, n_store=48, tight_ldc=True)


@pytest.mark.parametrize("M,N,K1", [(384, 384, 128), (1152, 128, 768)])
@pytest.mark.parametrize("epi", ["store_h16", "gelu_bwd"])
def test_gemm_stream_fused_down_projection(ctx, epi, M, N, K1):
    """down_out is null on this path (as the Swin layers call it): t is checked through the result."""
    c, ref = linear_case(epi, M, N, K1, 64, 6, "grid", ctx.prec, down=24, down_cols=64)
    out = run_linear(ctx, c, ref, route=4, cus=3, down_groups=1)
    check_linear(ctx, c, ref, out, route=4)


@pytest.mark.parametrize("bn,N", [(128, 384), (64, 64)])
def test_gemm_stream_continuous(ctx, bn, N):
    go(ctx, "store_h16", 384, N, 128, 0, route=4, bn=bn, cus=3, kind="continuous")


def test_forced_routes_launch_the_kernels_they_name(ctx, ctx32):
    """Each route runs the kernel it stands for (a forced route that quietly fell back to another kernel would make every case
    above check the wrong code)."""
    want = {1: {"gemm_nt_kernel<128, 128, 0>"}, 2: {"gemm256_kernel<256, 0>", "gemm256_kernel<128, 0>"}, 3: {"gemm_pp_kernel<0>"},
            4: {"gemm_stream_kernel<128, 0, false>"}}
    for route, names in want.items():
        got = profiled(ctx, lambda: go(ctx, "store_h16", 384, 256, 768, 64, route=route, cus=1))
        assert got == names, (route, got)
    assert profiled(ctx, lambda: go(ctx, "store_h16", 128, 64, 64, 0, route=1, bn=64)) == {"gemm_nt_kernel<128, 64, 0>"}
    assert profiled(ctx, lambda: go(ctx, "store_h16", 384, 64, 128, 0, route=4, bn=64, cus=3)) == {"gemm_stream_kernel<64, 0, false>"}
    c, ref = linear_case("store_h16", 384, 256, 768, 64, 5, "grid", ctx.prec, down=8, down_cols=16)
    assert profiled(ctx, lambda: run_linear(ctx, c, ref, route=3, cus=1, down_groups=1)) == {"gemm_pp_kernel<0, down 1>"}
    c, ref = linear_case("gelu_bwd", 384, 384, 128, 64, 6, "grid", ctx.prec, down=24, down_cols=64)
    assert profiled(ctx, lambda: run_linear(ctx, c, ref, route=4, cus=3, down_groups=1)) == {"gemm_stream_kernel<128, 3, true>"}
    assert profiled(ctx32, lambda: run_f32(ctx32, 64, 64, 16, big=1)) == {"gemm_f32_big_kernel"}
    assert profiled(ctx32, lambda: run_f32(ctx32, 130, 132, 772, big=0)) == {"gemm_f32_kernel"}


# ---- default routing: the ViT-B products at batch 2 (M = 512) -----------------------------------------------------------------
VITB = [("qkv", "store_h16", 2304, 768, 64), ("o", "store_h16", 768, 768, 64), ("fc1", "gelu", 3072, 768, 0),
        ("fc2", "resid_h16", 768, 3072, 64), ("fc2_dgrad", "gelu_bwd", 3072, 768, 64), ("fc1_dgrad", "store_h16", 768, 3072, 64)]


@pytest.mark.parametrize("name,epi,N,K1,K2", VITB, ids=[v[0] for v in VITB])
def test_default_route_vit_b_products(ctx, name, epi, N, K1, K2):
    go(ctx, epi, 512, N, K1, K2, route=0, seed=9)


# ---- patch epilogues --------------------------------------------------------------------------------------------------------
# image, patch, batch: Mvalid = 160 / 144 of M = 256 rows; 288 of 384 (a 256-row tile plus a 128-row tail on one workgroup)
GEOMS = {"img32": (32, 16, 40), "img64": (64, 16, 9), "img32_b72": (32, 16, 72)}
SMALL_GEOMS = ["img32", "img64"]


@functools.lru_cache(maxsize=None)
def patch_case(epi, geom, N, K, kind="grid", prec=None, row_scale=True, seed=0):
    img, ps, B = GEOMS[geom]
    g = img // ps
    patches, T = g * g, g * g + 1
    Mvalid = B * patches
    M = (Mvalid + 127) // 128 * 128
    gen = torch.Generator().manual_seed(2000 + seed)
    dtype = G.DTYPES[prec] if prec else torch.float64
    if kind == "grid":
        mk = lambda shape: G.grid(gen, shape)
    else:
        mk = lambda shape: (2 * torch.rand(shape, generator=gen) - 1).to(dtype)
    c = Case(epi=epi, A1=None, W1=mk((N, K)), M=M, Mvalid=Mvalid, patches=patches, psize=ps)
    if epi == "patch_fwd":
        c.A1 = mk((M, K))
        c.bias = G.grid(gen, (N,))
        c.pos = G.grid(gen, (T, N)) + torch.arange(T, dtype=torch.float64)[:, None]      # nonzero, distinct per token
    else:
        c.A1 = mk((B * T, K))                      # token-major gradient rows; a_gather skips each image's CLS row
        c.a_gather = True
        c.inv_std = (2.0, 4.0, 0.5)
        if row_scale:
            c.row_scale = 2.0 ** -(torch.arange(B) % 4).double()
        if epi == "patch_pgd":
            x0 = torch.randint(0, 65, (B, 3, img, img), generator=gen).double() / 64
            c.R = x0
            c.adv = (x0 + torch.randint(-8, 9, x0.shape, generator=gen).double() / 64).clamp(0, 1)
            c.pgd = (0.125, 1.0 / 32, 0.0, 1.0)
    ref = G.reference(c, torch.float16)
    if kind == "grid":
        G.exact_guard(ref["abs_z"], 2.0 ** -6)        # (inv_std, row_scale and the PGD constants are powers of two / on a binary grid)
    return c, ref


def run_patch(ctx, c, ref, *, route, cus=None, pad=8, expect_flag=0, poison=False):
    dt = ctx.dtype
    e = c.epi
    img, ps = int(round(c.patches ** 0.5)) * c.psize, c.psize
    g = img // ps
    B, T = c.Mvalid // c.patches, c.patches + 1
    N, K = c.W1.shape
    cs = ctx.CaseT()
    cs.M, cs.N, cs.K1, cs.epi, cs.bn, cs.route, cs.Mvalid = c.M, N, K, G.EPI[e], 128, route, c.Mvalid
    cs.tokens, cs.patches, cs.grid, cs.psize, cs.img = T, c.patches, g, ps, img
    A1 = c.A1.clone()
    if poison:
        A1[T + 2, 5] = float("inf")               # one infinite operand in a gathered (non-CLS) row
    a1 = dev_in(A1, dt, K + pad, rows=max(A1.shape[0], c.M)); cs.A1, cs.lda1 = ptr(a1), K + pad
    if e == "patch_fwd":
        a1[c.Mvalid:, :K] = 1.0                    # rows past Mvalid are computed (finite) but must not be stored
    w1 = dev_in(c.W1, dt, K + pad); cs.W1, cs.ldw1 = ptr(w1), K + pad
    keep = [a1, w1]
    if e == "patch_fwd":
        ldc = N + pad
        b = c.bias.float().cuda(); cs.bias = ptr(b)
        pos = dev_in(c.pos, torch.float32, ldc); cs.pos = ptr(pos)       # pos shares the pitch of C
        Cbuf = sentinel_buf(B * T + 16, ldc, dt)
        cs.C, cs.ldc = ptr(Cbuf), ldc
        keep += [b, pos]
    else:
        cs.a_gather = 1
        for k in range(3):
            cs.inv_std[k] = c.inv_std[k]
        if c.row_scale is not None:
            rs = c.row_scale.float().cuda(); cs.row_scale = ptr(rs); keep.append(rs)
        n_img = B * 3 * img * img
        Cbuf = sentinel_buf(1, n_img + 4096, torch.float32)
        cs.C = ptr(Cbuf)
        if e == "patch_pgd":
            Cbuf[0, :n_img] = c.adv.float().flatten().cuda()
            x0 = c.R.float().contiguous().cuda(); cs.R = ptr(x0); keep.append(x0)
            cs.pgd_eps, cs.pgd_alpha, cs.pgd_lo, cs.pgd_hi = c.pgd
    assert ctx.lib.vl_check_errors(ctx.h, ctx.stream()) == 0          # the error word is clear before the run
    with ctx.cus(cus):
        rc = ctx.lib.vl_debug_gemm(ctx.h, C.byref(cs), ctx.stream())
        sync()
    assert rc == 0, (rc, ctx.lib.vl_last_error())
    assert ctx.lib.vl_check_errors(ctx.h, ctx.stream()) == expect_flag   # untouched by a finite gradient, 2 -> VL_ERR_NONFINITE
    if e == "patch_fwd":
        written = ~torch.isnan(ref["C"][:, 0])                         # token rows of the B images; CLS rows stay
        live = torch.zeros_like(Cbuf, dtype=torch.bool)
        live[:B * T, :N] = written[:, None].cuda()
        assert bool(untouched(Cbuf)[~live].all()), "patch_fwd wrote outside the token rows below Mvalid"
        return Cbuf[:B * T, :N].cpu()[written], written
    assert bool(untouched(Cbuf)[0, n_img:].all()), "patch gradient wrote past the last image"
    return Cbuf[0, :n_img].cpu().view(B, 3, img, img), None


@pytest.mark.parametrize("geom", SMALL_GEOMS)
@pytest.mark.parametrize("route,N", [(1, 128), (0, 128), (2, 256)])
def test_patch_fwd(ctx, route, N, geom):
    c, ref = patch_case("patch_fwd", geom, N, 768)
    got, written = run_patch(ctx, c, ref, route=route, cus=3 if route == 2 else None)
    n, where = G.compare_exact(got, ref["C"][written], ctx.dtype)
    assert n == 0, (n, where)


def test_patch_fwd_on_both_tile_heights_of_gemm256(ctx):
    """M = 384 on ONE workgroup: a 256-row tile and the 128-row tail launch; Mvalid = 288 ends inside the tail."""
    c, ref = patch_case("patch_fwd", "img32_b72", 256, 768)
    names = profiled(ctx, lambda: run_patch(ctx, c, ref, route=2, cus=1))
    assert {"gemm256_kernel<256, 4>", "gemm256_kernel<128, 4>"} <= names, names


@pytest.mark.parametrize("geom", SMALL_GEOMS)
@pytest.mark.parametrize("row_scale", [True, False])
@pytest.mark.parametrize("route", [1, 2, 0])
@pytest.mark.parametrize("epi", ["patch_bwd", "patch_pgd"])
def test_patch_gradient_epilogues(ctx, epi, route, row_scale, geom):
    c, ref = patch_case(epi, geom, 768, 128, row_scale=row_scale)
    got, _ = run_patch(ctx, c, ref, route=route, cus=3 if route == 2 else None)
    n, where = G.compare_exact(got, ref["C"], torch.float32, signed_zero=epi != "patch_pgd")
    assert n == 0, (n, where)


@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("epi", ["patch_bwd", "patch_pgd"])
def test_patch_gradient_flags_a_non_finite_operand(ctx, epi, route):
    """One infinite operand: an ordinary data-dependent branch sets the error word to 2 (reported as VL_ERR_NONFINITE)."""
    c, ref = patch_case(epi, "img32", 768, 128)
    run_patch(ctx, c, ref, route=route, expect_flag=VL_ERR_NONFINITE, poison=True)
    assert ctx.lib.vl_check_errors(ctx.h, ctx.stream()) == 0           # reported once, then clear


@pytest.mark.parametrize("route", [1, 2])
def test_patch_pgd_continuous_sign_rule(ctx, route):
    """uniform(-1, 1) operands: where |g_ref| <= E the kernel's sign may differ, and the element may take either outcome."""
    c, ref = patch_case("patch_pgd", "img32", 768, 128, kind="continuous", prec=ctx.prec)
    E = G.sum_bound(ref["abs"], 128)
    unsure = ref["g"].abs() <= E
    assert float(unsure.double().mean()) <= 0.005, float(unsure.double().mean())      # on the reference alone
    got, _ = run_patch(ctx, c, ref, route=route)
    got = got.double()
    ok = (got == ref["C"]) | (unsure & ((got == ref["C_plus"]) | (got == ref["C_minus"])))
    assert bool(ok.all()), (int((~ok).sum()), torch.nonzero(~ok)[:5].tolist())


# ---- fp32 parity-mode GEMM ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def f32_operands(M, N, K, kind="grid", seed=0):
    gen = torch.Generator().manual_seed(3000 + seed)
    if kind == "grid":
        return G.grid(gen, (M + M // 4 + 2, K)), G.grid(gen, (N, K)), G.grid(gen, (N,)), G.grid(gen, (M, N))
    return (torch.randn(M, K, generator=gen), 0.05 * torch.randn(N, K, generator=gen), 0.1 * torch.randn(N, generator=gen),
            torch.randn(M, N, generator=gen))


def run_f32(ctx32, M, N, K, *, big, transA=False, transW=False, alpha=1.0, bias=True, resid=False, Mstore=0, gather=0,
            kind="grid", expect=0, pad=4):
    A, W, b, R = f32_operands(M, N, K, kind)
    A, W, b, R = A.float(), W.float(), b.float(), R.float()
    rows = torch.arange(M)
    if gather:
        rows = rows + rows // gather + 1             # row m reads token row m + m / patches + 1
    Aused = A[rows] if gather else A[:M]
    a_dev = dev_in((A if gather else A[:M]).T.contiguous() if transA else (A if gather else A[:M]), torch.float32,
                   (M if transA else K) + pad)
    w_dev = dev_in(W.T.contiguous() if transW else W, torch.float32, (N if transW else K) + pad)
    cs = ctx32.CaseT()
    cs.M, cs.N, cs.K1, cs.f32_big, cs.transA, cs.transW, cs.alpha, cs.Mstore = M, N, K, int(big), int(transA), int(transW), alpha, Mstore
    cs.A1, cs.lda1, cs.W1, cs.ldw1 = ptr(a_dev), a_dev.shape[1], ptr(w_dev), w_dev.shape[1]
    cs.a_gather, cs.patches = int(bool(gather)), gather
    ldc = N + pad
    Cbuf = sentinel_buf(M + 8, ldc, torch.float32)
    cs.C, cs.ldc = ptr(Cbuf), ldc
    b_dev = b.cuda()
    if bias:
        cs.bias = ptr(b_dev)
    ms = Mstore or M
    if resid:                                        # R aliases C
        Cbuf[:ms, :N] = R[:ms].cuda()
        cs.R, cs.ldr = ptr(Cbuf), ldc
    rc = ctx32.lib.vl_debug_gemm(ctx32.h, C.byref(cs), ctx32.stream())
    sync()
    assert rc == expect, (rc, ctx32.lib.vl_last_error())
    if rc != 0:
        assert bool(untouched(Cbuf)[:, N:].all()) and bool(untouched(Cbuf)[ms:].all())
        return
    live = torch.zeros_like(Cbuf, dtype=torch.bool)
    live[:ms, :N] = True
    assert bool(untouched(Cbuf)[~live].all()), "fp32 GEMM wrote outside Mstore x N"
    got = Cbuf[:ms, :N].cpu()
    ab = alpha * (Aused.double().abs() @ W.double().abs().T)
    ref = alpha * (Aused.double() @ W.double().T + 0.0)          # (+0 accumulator, as in gemm_ref.reference)
    if bias:
        ref, ab = ref + b.double(), ab + b.double().abs()
    if resid:
        ref, ab = ref + R.double(), ab + R.double().abs()
    ref, ab = ref[:ms], ab[:ms]
    if kind == "grid":
        G.exact_guard(ab, 2.0 ** -7)
        n, where = G.compare_exact(got, ref, torch.float32)
        assert n == 0, (n, where)
    else:
        n, where, ratio = G.compare_bounded(got, ref, G.sum_bound(ab, K))
        note_ratio("gemm_f32_big" if big else "gemm_f32", "f32", "continuous", ratio)
        assert n == 0, (n, where)


F32_SHAPES = [(64, 64, 16), (65, 68, 20), (130, 132, 772), (128, 128, 4)]


@pytest.mark.parametrize("big", [0, 1])
@pytest.mark.parametrize("shape", F32_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_f32_shapes_and_operand_layouts(ctx32, shape, big):
    M, N, K = shape
    run_f32(ctx32, M, N, K, big=big)
    run_f32(ctx32, M, N, K, big=big, transW=True)
    if M % 4 == 0:
        run_f32(ctx32, M, N, K, big=big, transA=True)
        run_f32(ctx32, M, N, K, big=big, transA=True, transW=True)
    else:
        # a transposed A is read four rows at a time: M must be a multiple of 4 (f32_kernels.h); the entry refuses, and the
        # next multiple of 4 runs instead
        run_f32(ctx32, M, N, K, big=big, transA=True, expect=VL_ERR_ARG)
        M4 = M + 4 - M % 4
        run_f32(ctx32, M4, N, K, big=big, transA=True)
        run_f32(ctx32, M4, N, K, big=big, transA=True, transW=True)


@pytest.mark.parametrize("big", [0, 1])
def test_gemm_f32_alpha_bias_residual_mstore_gather(ctx32, big):
    run_f32(ctx32, 130, 132, 772, big=big, alpha=0.5)
    run_f32(ctx32, 130, 132, 772, big=big, alpha=0.5, bias=False, resid=True)
    run_f32(ctx32, 130, 132, 772, big=big, bias=False)
    run_f32(ctx32, 65, 68, 20, big=big, resid=True, transW=True)
    run_f32(ctx32, 130, 132, 772, big=big, resid=True, Mstore=70)
    run_f32(ctx32, 64, 64, 16, big=big, Mstore=33)
    run_f32(ctx32, 128, 128, 4, big=big, gather=4, resid=True)
    run_f32(ctx32, 65, 68, 20, big=big, gather=4)


@pytest.mark.parametrize("big", [0, 1])
def test_gemm_f32_continuous(ctx32, big):
    run_f32(ctx32, 130, 132, 772, big=big, kind="continuous", resid=True)


# ---- refusals: return codes only, nothing launched ------------------------------------------------------------------------------
def refusal_case(ctx, M=128, N=256, K1=768, K2=0, epi="store_h16", route=1):
    dt = ctx.dtype
    bufs = dict(a=torch.zeros(M, K1 + 8, dtype=dt, device="cuda"), w=torch.zeros(N, K1 + 8, dtype=dt, device="cuda"),
                a2=torch.zeros(M, 64, dtype=dt, device="cuda"), w2=torch.zeros(N, 64, dtype=dt, device="cuda"),
                r=torch.zeros(M, N, dtype=torch.float32, device="cuda"), c=sentinel_buf(M, N, torch.float32 if epi in G.F32_OUT else dt),
                dw=torch.zeros(64, K1 + 8, dtype=dt, device="cuda"))
    cs = ctx.CaseT()
    cs.M, cs.N, cs.K1, cs.K2, cs.epi, cs.bn, cs.route = M, N, K1, K2, G.EPI[epi], 128, route
    cs.A1, cs.lda1, cs.W1, cs.ldw1 = ptr(bufs["a"]), K1 + 8, ptr(bufs["w"]), K1 + 8
    if K2:
        cs.A2, cs.lda2, cs.W2, cs.ldw2 = ptr(bufs["a2"]), 64, ptr(bufs["w2"]), 64
    cs.C, cs.ldc, cs.R, cs.ldr = ptr(bufs["c"]), N, ptr(bufs["r"]), N
    return cs, bufs


def refused(ctx, cs, bufs, code):
    rc = ctx.lib.vl_debug_gemm(ctx.h, C.byref(cs), ctx.stream())
    sync()
    assert rc == code, (rc, ctx.lib.vl_last_error())
    assert bool(untouched(bufs["c"]).all()), "a refused case wrote output"


def test_refuses_bad_arguments(ctx):
    cs, b = refusal_case(ctx)
    cs.A1 = ptr(b["a"]) + 2                                     # misaligned base pointer
    refused(ctx, cs, b, VL_ERR_ARG)
    cs, b = refusal_case(ctx)
    cs.lda1 = 768 + 4                                           # row pitch not a multiple of 16 bytes
    refused(ctx, cs, b, VL_ERR_ARG)
    cs, b = refusal_case(ctx, K1=96)                            # K1 % 64 != 0
    refused(ctx, cs, b, VL_ERR_ARG)
    cs, b = refusal_case(ctx)
    cs.n_store = 24                                             # not a multiple of 16
    refused(ctx, cs, b, VL_ERR_ARG)
    cs, b = refusal_case(ctx)
    cs.C = None                                                 # a required pointer
    refused(ctx, cs, b, VL_ERR_ARG)
    cs, b = refusal_case(ctx, M=192)                            # M % 128 != 0
    refused(ctx, cs, b, VL_ERR_ARG)


def test_refuses_routes_that_cannot_run_the_case(ctx):
    cs, b = refusal_case(ctx, K1=704, route=3)                  # ping-pong needs K1 / 64 >= STATIC_STEPS + 2 = 12
    refused(ctx, cs, b, VL_ERR_UNSUPPORTED)
    cs, b = refusal_case(ctx, K1=64, route=2)                   # gemm256 needs two K tiles
    refused(ctx, cs, b, VL_ERR_UNSUPPORTED)
    cs, b = refusal_case(ctx, K1=128, epi="resid_f32", route=4) # no fp32 residual epilogue in the streaming kernel
    refused(ctx, cs, b, VL_ERR_UNSUPPORTED)
    cs, b = refusal_case(ctx, K1=768, K2=64, route=1)           # a fused-down argument set sent to the 128-row kernel:
    cs.A2, cs.down_W, cs.down_ldw, cs.down_groups = None, ptr(b["dw"]), 768 + 8, 1     # launch_gemm would abort() on it
    refused(ctx, cs, b, VL_ERR_UNSUPPORTED)
    cs, b = refusal_case(ctx, K1=128, K2=64, route=0)           # ... and by default routing, where no kernel that fuses takes K1 = 128
    cs.A2, cs.down_W, cs.down_ldw, cs.down_groups = None, ptr(b["dw"]), 128 + 8, 1
    refused(ctx, cs, b, VL_ERR_UNSUPPORTED)
