"""Swin-T + LoRA on the vl_swin_* path (BASELINE config 4) against HF's SwinForImageClassification built from a local
SwinConfig (random init; no reference code exists for this model -- SURVEY 8c names this class as the oracle).  fp32 path:
held to 1e-4 (north_star allows 1e-3).  LoRA = plain-torch low-rank branches around HF's own nn.Linear modules (G5 style)."""
import importlib

import pytest
import torch
import torch.nn.functional as F

from helpers import O, PKG, pkg, rel_l2

pytestmark = pytest.mark.gpu

MEAN = torch.tensor(O.IMAGENET_MEAN).view(1, 3, 1, 1)
STD = torch.tensor(O.IMAGENET_STD).view(1, 3, 1, 1)
TARGETS = ("q", "k", "v", "o", "fc2")
HF_ATTR = {"q": ("attention", "q_proj"), "k": ("attention", "k_proj"), "v": ("attention", "v_proj"), "o": ("attention", "o_proj"),
           "fc1": ("mlp", "fc1"), "fc2": ("mlp", "fc2")}


class LoraLinear(torch.nn.Module):
    def __init__(self, base, A, B, scaling):
        super().__init__()
        self.base, self.A, self.B, self.scaling = base, A, B, scaling

    def forward(self, x):
        return self.base(x) + self.scaling * F.linear(F.linear(x, self.A), self.B)


def hf_swin(num_labels, seed, depths=(2, 2, 6, 2)):
    from transformers import SwinConfig, SwinForImageClassification
    torch.manual_seed(seed)
    cfg = SwinConfig(num_labels=num_labels, depths=list(depths))
    cfg._attn_implementation = "eager"
    m = SwinForImageClassification(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                                   # HF initialises bias tables / LayerNorms trivially: make every term count
        for n, p in m.named_parameters():
            if "relative_position_bias_table" in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            elif n.endswith("norm.weight") or "layernorm" in n and n.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            elif p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return m


def add_lora(m, r, alpha, seed):
    g = torch.Generator().manual_seed(seed)
    ab = {}
    for si, stage in enumerate(m.swin.encoder.layers):
        for bi, blk in enumerate(stage.blocks):
            for t in TARGETS:
                parent = getattr(blk, HF_ATTR[t][0])
                base = getattr(parent, HF_ATTR[t][1])
                A = (torch.rand(r, base.in_features, generator=g) * 2 - 1) / base.in_features ** 0.5
                B = torch.randn(base.out_features, r, generator=g) * 0.05
                setattr(parent, HF_ATTR[t][1], LoraLinear(base, A, B, alpha / r))
                ab[(si, bi, t)] = (A, B)
    return ab


def make_engine(m, num_labels, r=0, ab=None, depths=(2, 2, 6, 2), precision="f32"):
    swin = importlib.import_module(PKG + ".swin")
    eng = swin.SwinEngine(swin.SwinArch(num_labels=num_labels, depths=tuple(depths)), lora_r=r, lora_alpha=16.0, lora_targets=TARGETS if r else (),
                          precision=precision)
    sd = {k.replace(".base.", "."): v for k, v in m.state_dict().items() if not k.endswith((".A", ".B"))}
    eng.load_state_dict(sd)
    if ab:
        for (si, bi, t), (A, B) in ab.items():
            eng.param(si, bi, t, "A").copy_(A)
            eng.param(si, bi, t, "B").copy_(B)
    return eng


TOL_LOGITS = {"f32": 1e-4, "f16": 4e-3}       # north_star: 1e-3 fp32 / 1e-2 16-bit
TOL_GRAD = {"f32": 1e-4, "f16": 6e-3}


@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("r", [0, 16])
def test_swin_t_logits_loss_and_input_gradient(r, prec):
    torch.set_num_threads(16)
    m = hf_swin(10, seed=3)
    ab = add_lora(m, r, 16.0, seed=5) if r else None
    eng = make_engine(m, 10, r, ab, precision=prec)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(3, 3, 224, 224, generator=g)
    y = torch.randint(0, 10, (3,), generator=g)
    logits = eng.forward(x.cuda(), normalise=True).cpu()
    loss = eng.loss_ce(y.cuda()).item()
    gx = eng.backward_input(tuple(x.shape)).cpu()
    xr = x.clone().requires_grad_(True)
    ref_logits = m((xr - MEAN) / STD).logits
    ref_loss = F.cross_entropy(ref_logits, y)
    (g_ref,) = torch.autograd.grad(ref_loss, xr)
    assert rel_l2(logits, ref_logits.detach()) < TOL_LOGITS[prec], rel_l2(logits, ref_logits.detach())
    assert abs(loss - ref_loss.item()) < TOL_LOGITS[prec] * ref_loss.item()
    assert rel_l2(gx, g_ref) < TOL_GRAD[prec], rel_l2(gx, g_ref)
    if r:       # the adapters matter in this case
        eng0 = make_engine(m, 10, 0, None)
        assert rel_l2(eng0.forward(x.cuda(), normalise=True).cpu(), ref_logits.detach()) > 1e-2


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_swin_shallow_variant_and_pgd_matches_torch_loop(prec):
    """depths (1, 1, 2, 1): odd / even block positions, shifted and unshifted windows in every stage that has them; PGD-3 of
    vl_swin_pgd_attack against the same loop written with torch autograd on the HF model (canonical PGD)."""
    torch.set_num_threads(16)
    depths = (1, 2, 2, 1)
    m = hf_swin(12, seed=13, depths=depths)
    ab = add_lora(m, 8, 16.0, seed=15)
    eng = make_engine(m, 12, 8, ab, depths=depths, precision=prec)
    g = torch.Generator().manual_seed(19)
    x = torch.rand(2, 3, 224, 224, generator=g)
    y = torch.randint(0, 12, (2,), generator=g)
    eps, alpha, steps = 8 / 255, 2 / 255, 3
    adv = eng.pgd_attack(x.cuda(), y.cuda(), eps, alpha, steps, random_start=False).cpu()
    ref = x.clone()
    for _ in range(steps):
        xr = ref.clone().requires_grad_(True)
        (gr,) = torch.autograd.grad(F.cross_entropy(m((xr - MEAN) / STD).logits, y), xr)
        ref = O.pgd_step(ref, x, gr, eps, alpha)
    same = ((adv - ref).abs() < 1e-6).float().mean().item()
    assert same > (0.999 if prec == "f32" else 0.99), same          # 16-bit: near-zero gradient entries may flip their sign
    assert (adv - x).abs().max().item() <= eps + 1e-6 and adv.min().item() >= 0 and adv.max().item() <= 1
    # seeded random start, determinism
    a1 = eng.pgd_attack(x.cuda(), y.cuda(), eps, alpha, 2, random_start=True, seed=4)
    a2 = eng.pgd_attack(x.cuda(), y.cuda(), eps, alpha, 2, random_start=True, seed=4)
    assert torch.equal(a1, a2)


def test_swin_refuses_unsupported_shapes():
    P = pkg()
    swin = importlib.import_module(PKG + ".swin")
    with pytest.raises(P.VitLoraError):
        swin.SwinEngine(swin.SwinArch(image_size=200))              # 50 x 50 tokens: not a multiple of the window
    with pytest.raises(P.VitLoraError):
        swin.SwinEngine(swin.SwinArch(heads=(4, 6, 12, 24)))        # head_dim != 32


def test_swin_fp16_backward_out_of_range_is_flagged_as_nonfinite_not_as_a_bad_label():
    """Round-3 ADVICE: the Swin fp16 path shares the ViT path's saturate-and-flag backward kernels, but its API mapped ANY flag
    to "label outside [0, num_labels)".  LayerNorm gains of 512 per block cannot fit fp16 over 12 blocks: backward_input and
    the PGD attack must report NonFiniteGradient (VL_ERR_NONFINITE) through SwinEngine.check(), the flag is cleared by reading
    it, a bad label is still reported as VitLoraError, and the fp32 mode has the range."""
    P = pkg()
    m = hf_swin(10, seed=41, depths=(2, 2, 2, 2))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "layernorm" in n and n.endswith("weight"):
                p.mul_(512.0)
    g = torch.Generator().manual_seed(43)
    x = torch.rand(2, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 10, (2,), generator=g).cuda()
    eng = make_engine(m, 10, depths=(2, 2, 2, 2), precision="f16")
    eng.forward(x, normalise=True)
    eng.loss_ce(y)
    eng.backward_input(tuple(x.shape))
    with pytest.raises(P.NonFiniteGradient):
        eng.check()
    eng.check()                                  # cleared by reading it
    eng.pgd_attack(x, y, 8 / 255, 2 / 255, 2, random_start=False)
    with pytest.raises(P.NonFiniteGradient):
        eng.check()
    # a label outside the range is still its own error
    eng.forward(x, normalise=True)
    eng.loss_ce(torch.tensor([3, 10], device="cuda"))
    with pytest.raises(P.VitLoraError) as ei:
        eng.check()
    assert not isinstance(ei.value, P.NonFiniteGradient)
    e32 = make_engine(m, 10, depths=(2, 2, 2, 2), precision="f32")
    e32.forward(x, normalise=True)
    e32.loss_ce(y)
    g32 = e32.backward_input(tuple(x.shape))
    e32.check()
    assert torch.isfinite(g32).all()


def test_swin_two_chain_attack_equals_the_single_chain_attack(monkeypatch):
    """vl_swin_pgd_attack runs batches of >= 32 images as two half-batch chains on two streams (round 5; shallow copies of the
    handle whose workspaces share the planned bytes).  Images are independent and 1/B differs by a power of two between the forms,
    so the chained result must be the single-chain result bit for bit -- here at batch 8 (threshold lowered to 2) with LoRA,
    random start (drawn over the whole batch in both forms) and at an odd batch 7 (4 + 3: 1/B is no power-of-two multiple, so only
    agreement to rounding is asked there); a forward / backward pair after a chained attack works on the main workspace again."""
    depths = (1, 1, 2, 1)
    m = hf_swin(12, seed=41, depths=depths)
    ab = add_lora(m, 8, 16.0, seed=42)
    g = torch.Generator().manual_seed(43)
    x = torch.rand(8, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 12, (8,), generator=g).cuda()
    outs = {}
    for mode in ("0", "2", "3"):
        monkeypatch.setenv("VITLORA_SWIN_CHAINS", mode)
        monkeypatch.setenv("VITLORA_SWIN_CHAIN_MIN", "2")
        eng = make_engine(m, 12, 8, ab, depths=depths, precision="f16")
        a8 = eng.pgd_attack(x, y, 8 / 255, 2 / 255, 3, random_start=True, seed=5).clone()
        a7 = eng.pgd_attack(x[:7].contiguous(), y[:7].contiguous(), 8 / 255, 2 / 255, 3, random_start=False).clone()
        logits = eng.forward(x, normalise=True).clone()          # the main workspace after a chained attack
        eng.loss_ce(y)
        gx = eng.backward_input(tuple(x.shape)).clone()
        eng.check()
        torch.cuda.synchronize()
        outs[mode] = (a8.cpu(), a7.cpu(), logits.cpu(), gx.cpu())
        del eng
    assert torch.equal(outs["0"][0], outs["2"][0]), float((outs["0"][0] != outs["2"][0]).float().mean())
    for k in ("2", "3"):           # 4 + 3 and 3 + 3 + 2 / 3 + 2 + 2 images: 1 / B is no power-of-two multiple of the single chain's
        assert float((outs["0"][0] == outs[k][0]).float().mean()) > 0.995 and float((outs["0"][1] == outs[k][1]).float().mean()) > 0.995
        assert torch.equal(outs["0"][2], outs[k][2]) and torch.equal(outs["0"][3], outs[k][3])


def test_swin_normalisation_set_after_the_plan_reaches_the_chains(monkeypatch):
    """vl_swin_set_normalization AFTER the chain workspaces exist (one chained attack has run): the next chained attack uses the
    new constants -- bit for bit the result of an engine without chains under the same constants at batch 8 (4 + 4: 1/B differs
    by a power of two), and not the result under the default constants."""
    import ctypes as C
    depths = (1, 1, 2, 1)
    m = hf_swin(12, seed=41, depths=depths)
    ab = add_lora(m, 8, 16.0, seed=42)
    g = torch.Generator().manual_seed(43)
    x = torch.rand(8, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 12, (8,), generator=g).cuda()
    mean, std = (C.c_float * 3)(0.40, 0.50, 0.45), (C.c_float * 3)(0.30, 0.25, 0.20)
    monkeypatch.setenv("VITLORA_SWIN_CHAIN_MIN", "2")
    outs = {}
    for mode in ("2", "0"):
        monkeypatch.setenv("VITLORA_SWIN_CHAINS", mode)
        eng = make_engine(m, 12, 8, ab, depths=depths, precision="f16")
        default = eng.pgd_attack(x, y, 8 / 255, 2 / 255, 3, random_start=True, seed=5).clone()
        assert eng.lib.vl_swin_set_normalization(eng.h, mean, std) == 0
        other = eng.pgd_attack(x, y, 8 / 255, 2 / 255, 3, random_start=True, seed=5).clone()
        eng.check()
        torch.cuda.synchronize()
        outs[mode] = (default.cpu(), other.cpu())
        del eng
    assert torch.equal(outs["2"][1], outs["0"][1]), float((outs["2"][1] != outs["0"][1]).float().mean())
    for mode in ("2", "0"):
        assert not torch.equal(outs[mode][0], outs[mode][1])


def test_swin_narrow_stage_mlp_matches_hf_at_a_ragged_batch():
    """Stage 1's MLP (C = 96: fc1 -> GELU -> fc2 forward, fc2 dgrad -> * gelu' -> fc1 dgrad backward, one GEMM launch per product)
    at depths (2, 1, 1, 1) with LoRA r = 16 on fc2 and an odd batch 3 = ragged last tile, fp16:
    logits and input gradient against HF Swin through the oracle tolerance, and a seeded PGD attack run twice on the same engine
    must reproduce itself bit for bit.  (Until the fused stage-1 MLP kernel was removed this case compared that kernel with the
    two-GEMM form; DESIGN.md section 6 keeps its measurements.)"""
    depths = (2, 1, 1, 1)
    m = hf_swin(12, seed=31, depths=depths)
    ab = add_lora(m, 16, 16.0, seed=32)
    g = torch.Generator().manual_seed(33)
    x = torch.rand(3, 3, 224, 224, generator=g)
    y = torch.randint(0, 12, (3,), generator=g)
    eng = make_engine(m, 12, 16, ab, depths=depths, precision="f16")
    l1 = eng.forward(x.cuda(), normalise=True).clone()
    eng.loss_ce(y.cuda())
    g1 = eng.backward_input(tuple(x.shape)).clone()
    a0 = eng.pgd_attack(x.cuda(), y.cuda(), 8 / 255, 2 / 255, 2, random_start=True, seed=2).clone()
    a1 = eng.pgd_attack(x.cuda(), y.cuda(), 8 / 255, 2 / 255, 2, random_start=True, seed=2).clone()
    eng.check()
    torch.cuda.synchronize()
    l1, g1 = l1.cpu(), g1.cpu()
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all()
    assert torch.equal(a0, a1), float((a0 != a1).float().mean())
    xr = x.clone().requires_grad_(True)
    ref_logits = m((xr - MEAN) / STD).logits
    (ref_g,) = torch.autograd.grad(F.cross_entropy(ref_logits, y), xr)
    assert rel_l2(l1, ref_logits.detach()) < TOL_LOGITS["f16"], rel_l2(l1, ref_logits.detach())
    assert rel_l2(g1, ref_g) < TOL_GRAD["f16"], rel_l2(g1, ref_g)


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_swin_workspace_is_never_written_outside_its_planned_bytes(prec):
    """Same guard-band check as the ViT engine's (tests/test_hip_engine.py): 1 MiB of pattern on both sides of the bytes
    vl_swin_plan asked for stays intact through forward / loss / input gradient / a PGD attack at an odd batch, and a second run
    over the used workspace reproduces the first bit for bit.  Round 5 (round-4 verdict 8): the results do not depend on what the
    planned bytes held at hand-over either -- a third run after the test has filled EVERY planned byte with 0xFF (NaN patterns
    in fp16 and fp32) reproduces the first bit for bit: pad columns are written by the kernels that own the rows, the K-tail
    heads of the unpadded stages are zeroed per forward (csrc/swin.hip: zero_tails_kernel), nothing else is read before it is
    written."""
    import ctypes as C
    depths = (1, 2, 2, 1)
    m = hf_swin(12, seed=13, depths=depths)
    ab = add_lora(m, 8, 16.0, seed=15)
    eng = make_engine(m, 12, 8, ab, depths=depths, precision=prec)
    g = torch.Generator().manual_seed(23)
    x = torch.rand(3, 3, 224, 224, generator=g)
    y = torch.randint(0, 12, (3,), generator=g)
    n = C.c_size_t()
    assert eng.lib.vl_swin_plan(eng.h, 3, C.byref(n)) == 0
    n = n.value
    guard = 1 << 20
    buf = torch.full((n + 2 * guard + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    base = (buf.data_ptr() + guard + 255) // 256 * 256
    off = base - buf.data_ptr()
    eng._ws, eng._plan = buf, 3
    assert eng.lib.vl_swin_set_workspace(eng.h, C.c_void_p(base), n) == 0
    outs = []
    for rep in range(3):
        if rep == 2:
            buf[off:off + n] = 0xFF          # a caller that reused the buffer between calls
            torch.cuda.synchronize()
        logits = eng.forward(x.cuda(), normalise=True).clone()
        loss = eng.loss_ce(y.cuda()).clone()
        gx = eng.backward_input(tuple(x.shape)).clone()
        adv = eng.pgd_attack(x.cuda(), y.cuda(), 8 / 255, 2 / 255, 2, random_start=True, seed=2).clone()
        torch.cuda.synchronize()
        outs.append((logits, loss, gx, adv))
        assert bool((buf[:off] == 0xA5).all()), (prec, "bytes BEFORE the workspace were written")
        bad = (buf[off + n:] != 0xA5).nonzero()
        assert bad.numel() == 0, (prec, "bytes AFTER the workspace were written", int(bad[0]), int(bad[-1]), int(bad.numel()))
    for rep in (1, 2):
        for k, (a, b) in enumerate(zip(outs[0], outs[rep])):
            assert not torch.isnan(b).any(), (prec, rep, k)
            assert torch.equal(a, b), (prec, rep, k, "run differs from the first", (a != b).sum().item())


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_swin_results_do_not_depend_on_what_the_previous_kernel_left_in_lds(prec):
    """As tests/test_hip_engine.py::test_results_do_not_depend_on_what_the_previous_kernel_left_in_lds: with the process-wide
    "poison_lds" hook (set through a ViT handle: include/vitlora.h) every GEMM / LayerNorm / window-attention launch of the Swin
    path starts on LDS full of NaN patterns; logits, input gradient and a PGD attack come out bit for bit as without it."""
    from helpers import make_case, make_engine as make_vit
    cfgv, wv, _, _, _ = make_case(batch=1, r=0)
    vit = make_vit(cfgv, wv)
    depths = (1, 2, 2, 1)
    m = hf_swin(12, seed=13, depths=depths)
    ab = add_lora(m, 8, 16.0, seed=15)
    eng = make_engine(m, 12, 8, ab, depths=depths, precision=prec)
    g = torch.Generator().manual_seed(29)
    x = torch.rand(3, 3, 224, 224, generator=g)
    y = torch.randint(0, 12, (3,), generator=g)
    outs = []
    n0 = vit.counter("lds_poisons")
    try:
        for poison in (0, 1):
            vit.set_option("poison_lds", poison)
            logits = eng.forward(x.cuda(), normalise=True).clone()
            eng.loss_ce(y.cuda())
            gx = eng.backward_input(tuple(x.shape)).clone()
            adv = eng.pgd_attack(x.cuda(), y.cuda(), 8 / 255, 2 / 255, 2, random_start=True, seed=2).clone()
            torch.cuda.synchronize()
            outs.append((logits, gx, adv))
    finally:
        vit.set_option("poison_lds", 0)
    assert vit.counter("lds_poisons") - n0 > 50
    for k, (a, b) in enumerate(zip(*outs)):
        assert not torch.isnan(b).any() and torch.equal(a, b), (prec, k, int((a != b).sum()))
