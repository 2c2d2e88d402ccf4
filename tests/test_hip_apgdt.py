"""GPU tests of APGD-T (targeted Auto-PGD on the DLR loss, L-inf): vl_dlr_targeted_loss, vl_apgd_targets, vl_apgdt_attack and the
APGDT / run_suite facade.

The reference is tests/apgdt_ref.py.  The loss kernel is held to its float32 restatement bit for bit,
the target kernel exactly; the whole attack is held to apgd_ref's state machine through its OWN trace and to properties checked
with the library's own forward (full-trajectory parity with the CPU oracle is not asked, as in tests/test_hip_apgd.py).  EPS,
STEPS and N_TARGET are apgdt_ref's, chosen on the CPU (tests/test_apgdt_ref_cpu.py)."""
import importlib
import os

import numpy as np
import pytest
import torch

import apgd_ref as A
import apgdt_ref as R
from helpers import O, PKG, make_case, make_engine, pkg

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS, STEPS, N_TARGET = R.CASE_EPS, R.CASE_STEPS, R.CASE_N_TARGET      # chosen on the CPU: tests/test_apgdt_ref_cpu.py
PRECS = ["f16", "bf16", "f32"]

# ---- shared case: make_case(batch=8, seed=5), labels = the clean argmax of the CPU oracle, image 0's label changed ----------------
_CASE, _ENG, _RUN = {}, {}, {}


def case():
    if not _CASE:
        cfg, w, lora, x, _ = make_case(batch=8, seed=5)
        clean = O.vit_forward(w, cfg, O.normalise(x), lora).argmax(1)
        y = clean.clone()
        y[0] = (y[0] + 1) % cfg.num_labels
        _CASE.update(cfg=cfg, w=w, lora=lora, x=x, y=y, clean=clean)
    return _CASE


def engine(prec):
    if prec not in _ENG:
        c = case()
        _ENG[prec] = make_engine(c["cfg"], c["w"], c["lora"], precision=prec)
    return _ENG[prec]


def cpu(r):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in r.items()}


def run(prec, **kw):
    """One traced attack on the shared case (computed once per key, never modified)."""
    key = (prec, tuple(sorted(kw.items())))
    if key not in _RUN:
        c = case()
        args = dict(steps=STEPS, n_target_classes=N_TARGET, n_restarts=1, trace=True)
        args.update(kw)
        _RUN[key] = cpu(engine(prec).apgdt_attack(c["x"].cuda(), c["y"].cuda(), EPS, **args))
    return _RUN[key]


def same(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not torch.equal(a[k], b[k])]


def check_result(eng, r, x, y, eps, runs):
    """The item-4 properties of a result dict (CPU tensors), checked with the library's own forward."""
    pred = eng.forward(r["x_adv"].cuda(), normalise=True).argmax(1).cpu()
    clean = eng.forward(x.cuda(), normalise=True).argmax(1).cpu()
    changed = (r["x_adv"] != x).flatten(1).any(1)
    assert torch.equal(r["clean_correct"], clean == y)
    assert (pred != y)[changed].all()                                   # every changed image is misclassified
    assert torch.equal(r["x_adv"][~changed], x[~changed])               # unchanged images are bit-equal to x0
    assert (r["x_adv"] - x).abs().max().item() <= eps + 1e-7
    assert not changed[~r["clean_correct"]].any()                       # clean-wrong images are untouched
    assert r["robust_run"].shape == (runs, x.shape[0]) and r["loss_best"].shape == (runs, x.shape[0])
    assert torch.equal(r["robust"], r["clean_correct"] & r["robust_run"].all(0))
    first = torch.where((~r["robust_run"]).any(0), (~r["robust_run"]).int().argmax(0), torch.full((x.shape[0],), -1)).int()
    assert torch.equal(r["fooled_by"], torch.where(r["clean_correct"], first, torch.full_like(first, -1)))
    assert torch.equal(changed, r["fooled_by"] >= 0)
    assert r["x_adv"].min().item() >= 0 and r["x_adv"].max().item() <= 1
    return changed


# ---- 1. the loss kernel, bit for bit -----------------------------------------------------------------------------------------------
def loss_rows(C):
    """B = 9 rows: the label at ranks 1, 2, 3, 4 and last, the target at various other ranks; row 5 has its four largest logits
    equal (label and target among them), row 6 two tied pairs, rows 7 and 8 are random."""
    g = torch.Generator().manual_seed(C)
    z = torch.randn(9, C, generator=g).numpy().astype(F32)
    z[5, [0, 1, C - 2, C - 1]] = 4.0
    z[6, [0, 2]] = 3.0
    z[6, [1, 3]] = 2.5
    rank_y = [0, 1, 2, 3, C - 1, 0, 2, 1, 3]
    rank_t = [1, 0, C - 1, 2, 0, 3, 3, C - 1, C // 2 if C // 2 != 3 else 0]
    y = np.array([R.order(z[b])[rank_y[b]] for b in range(9)])
    t = np.array([R.order(z[b])[rank_t[b]] for b in range(9)])
    assert (y != t).all()
    return z, y, t


@pytest.mark.parametrize("C", [4, 10, 21, 70, 130])
def test_dlr_loss_kernel_bit_exact(C):
    eng = engine("f16")
    z, y, t = loss_rows(C)
    want_l, want_g = R.dlr_targeted(z, y, t, F32)
    loss, d, err = eng.dlr_targeted_loss(torch.from_numpy(z), torch.from_numpy(y), torch.from_numpy(t))
    torch.cuda.synchronize()
    assert np.array_equal(loss.cpu().numpy(), want_l), (loss.cpu().numpy(), want_l)
    assert np.array_equal(d.cpu().numpy(), want_g), int((d.cpu().numpy() != want_g).sum())
    assert np.isfinite(loss.cpu().numpy()).all() and np.isfinite(d.cpu().numpy()).all()      # row 5: D = 1e-12
    assert int(err.item()) == 0


def test_dlr_loss_kernel_refuses_bad_labels_and_targets():
    eng = engine("f16")
    C = 10
    z, y, t = loss_rows(C)
    for row, (yb, tb), code in ((1, (C, 0), 1), (2, (-1, 0), 1), (3, (2, C), 6), (4, (2, -1), 6), (7, (5, 5), 6)):
        y2, t2 = y.copy(), t.copy()
        y2[row], t2[row] = yb, tb
        loss, d, err = eng.dlr_targeted_loss(torch.from_numpy(z), torch.from_numpy(y2), torch.from_numpy(t2))
        torch.cuda.synchronize()
        loss, d = loss.cpu().numpy(), d.cpu().numpy()
        assert int(err.item()) == code, (row, int(err.item()))
        assert np.isnan(loss[row]) and np.isnan(d[row]).all()
        keep = np.arange(9) != row
        want_l, want_g = R.dlr_targeted(z[keep], y[keep], t[keep], F32)
        assert np.array_equal(loss[keep], want_l) and np.array_equal(d[keep], want_g)
    # inside the attack the error word is the handle's: the next check reports it
    c = case()
    eng.check()
    bad = c["y"].clone().view(1, -1).int()                      # a target row equal to the labels
    eng.apgdt_attack(c["x"].cuda(), c["y"].cuda(), EPS, steps=1, n_target_classes=1, targets=bad)
    with pytest.raises(pkg().VitLoraError):
        eng.check()
    eng.check()                                                 # reported once


# ---- 2. the target kernel, exactly -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 10, 21, 70, 130])
def test_target_kernel_exact(C):
    eng = engine("f16")
    g = torch.Generator().manual_seed(100 + C)
    z = torch.randn(9, C, generator=g).numpy().astype(F32)
    z[1, :] = 1.0                                               # all tied
    z[2, [0, C - 1]] = z[2].max() + 1                           # a tied maximum: the first one is the prediction
    z[3, 1:4] = z[3, 0]                                         # ties below the maximum
    y = z.argmax(1)
    y[4] = (y[4] + 1) % C                                       # clean-wrong rows
    y[2] = C - 1                                                # the second of the tied maxima is not the prediction
    for n in sorted({1, min(3, C - 1), min(9, C - 1), C - 1}):
        tg, cc = eng.apgd_targets(torch.from_numpy(z), torch.from_numpy(y), n)
        torch.cuda.synchronize()
        assert np.array_equal(tg.cpu().numpy(), R.targets(z, y, n)), n
        assert np.array_equal(cc.cpu().numpy(), z.argmax(1) == y)
    assert not (z.argmax(1) == y)[[2, 4]].any()
    with pytest.raises(pkg().VitLoraError):
        eng.apgd_targets(torch.from_numpy(z), torch.from_numpy(y), C)


# ---- 3. the input gradient against the oracle ------------------------------------------------------------------------------------
def unit_err(got, ref):
    """Per image: both gradients scaled to unit L2 norm, the L2 norm of their difference; the maximum over the images."""
    g = got.double().flatten(1)
    r = ref.double().flatten(1)
    g, r = g / g.norm(dim=1, keepdim=True), r / r.norm(dim=1, keepdim=True)
    return float((g - r).norm(dim=1).max())


@pytest.mark.parametrize("prec", PRECS)
def test_input_gradient_of_the_dlr_loss_against_the_oracle(prec):
    """The DLR error may be at most twice the CE error measured here on the same case and precision: the backward chain is the
    same, only the dlogits row differs, and the factor covers the row's other conditioning.  Measured on MI355X (DLR / CE):
    f16 1.243e-3 / 1.292e-3, bf16 1.703e-2 / 1.080e-2, f32 1.264e-6 / 1.254e-6."""
    c, eng = case(), engine(prec)
    x, y = c["x"], c["clean"]                                   # labels = the clean argmax
    xr = x.clone().requires_grad_(True)
    logits_ref = O.vit_forward(c["w"], c["cfg"], O.normalise(xr), c["lora"])
    t = torch.from_numpy(R.targets(logits_ref.detach().numpy(), y.numpy(), 1)[0].astype(np.int64))
    (g_dlr,) = torch.autograd.grad(R.dlr_torch(logits_ref, y, t).sum(), xr, retain_graph=True)
    (g_ce,) = torch.autograd.grad(torch.nn.functional.cross_entropy(logits_ref, y, reduction="sum"), xr)
    # the library: forward -> dlr_targeted_loss -> set_dlogits -> backward to the input
    logits = eng.forward(x.cuda(), normalise=True)
    _, d, err = eng.dlr_targeted_loss(logits, y, t)
    eng.set_dlogits(d)
    got_dlr, _ = eng.backward(True, False, tuple(x.shape))
    # the existing path on the same case: forward -> loss_ce -> backward
    eng.forward(x.cuda(), normalise=True)
    eng.loss_ce(y.cuda())
    got_ce, _ = eng.backward(True, False, tuple(x.shape))
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    e_dlr, e_ce = unit_err(got_dlr.cpu(), g_dlr), unit_err(got_ce.cpu(), g_ce)
    print(f"{prec}: input-gradient error (unit-norm, max over images) DLR {e_dlr:.3e}, CE {e_ce:.3e}, ratio {e_dlr / e_ce:.2f}")
    assert e_dlr <= 2 * e_ce


# ---- 4. the whole attack: its own trace and the properties of x_adv ------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_attack_is_the_state_machine_on_its_own_trace_and_x_adv_holds_its_properties(prec):
    c, r, eng = case(), run(prec), engine(prec)
    step, _, best, robust = A.replay(r["trace_loss"].numpy(), r["trace_pred"].numpy(), EPS)
    assert np.array_equal(r["trace_step"].numpy(), step)
    assert np.array_equal(r["loss_best"][-1].numpy(), best)
    assert np.array_equal(r["robust_run"][-1].numpy(), robust)
    changed = check_result(eng, r, c["x"], c["y"], EPS, N_TARGET)
    print(f"{prec}: fooled_by {r['fooled_by'].tolist()}, robust {r['robust'].int().tolist()}")
    assert changed.any()
    assert not changed[0]
    if prec == "f32":
        want = R.targets(O.vit_forward(c["w"], c["cfg"], O.normalise(c["x"]), c["lora"]).detach().numpy(), c["y"].numpy(), N_TARGET)
        assert np.array_equal(r["targets"].numpy(), want)


# ---- 5. the fold and the run loop ------------------------------------------------------------------------------------------------
def test_one_call_equals_the_host_side_fold_of_single_run_calls():
    """Targets given in the order (9th, 5th, 1st most likely wrong class), so that later runs have something left to fool."""
    c, eng = case(), engine("f16")
    x, y = c["x"].cuda(), c["y"].cuda()
    table = eng.apgdt_attack(x, y, EPS, steps=1, n_target_classes=9)["targets"][[8, 4, 0]].clone()
    K, Rn, seed = 3, 2, 11
    one = cpu(eng.apgdt_attack(x, y, EPS, steps=STEPS, n_target_classes=K, n_restarts=Rn, seed=seed, targets=table, trace=True))
    x_adv, still, fooled_by = c["x"].clone(), one["clean_correct"].clone(), torch.full((8,), -1, dtype=torch.int32)
    for k in range(K):
        for r in range(Rn):
            i = k * Rn + r
            s = cpu(eng.apgdt_attack(x, y, EPS, steps=STEPS, n_target_classes=1, n_restarts=1, seed=seed + i, targets=table[k:k + 1],
                                     trace=True))
            assert torch.equal(s["loss_best"][0], one["loss_best"][i]) and torch.equal(s["robust_run"][0], one["robust_run"][i]), i
            take = still & ~s["robust_run"][0]
            assert torch.equal(s["fooled_by"] == 0, s["clean_correct"] & ~s["robust_run"][0])
            x_adv[take] = s["x_adv"][take]
            fooled_by[take] = i
            still &= s["robust_run"][0]
    for k in ("trace_loss", "trace_step", "trace_pred"):
        assert torch.equal(s[k], one[k]), k                     # the trace is the last run's
    assert torch.equal(one["x_adv"], x_adv) and torch.equal(one["robust"], still) and torch.equal(one["fooled_by"], fooled_by)
    assert torch.equal(one["targets"], table.cpu())
    print(f"fooled_by {fooled_by.tolist()}")
    check_result(eng, one, c["x"], c["y"], EPS, K * Rn)
    assert not torch.equal(one["loss_best"][0], one["loss_best"][1])      # a restart is another start point


# ---- 6. graphs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_graph_is_reused_equals_eager_and_apgd_ce_in_between_changes_nothing(prec):
    c, r, eng = case(), run(prec), engine(prec)
    x, y = c["x"].cuda(), c["y"].cuda()
    kw = dict(steps=STEPS, n_target_classes=N_TARGET, trace=True)
    eng.apgdt_attack(x, y, EPS, **kw)                           # (make this key's scratch and graph current)
    before = eng.counter("graph_captures")
    again = cpu(eng.apgdt_attack(x, y, EPS, **kw))
    assert eng.counter("graph_captures") == before              # every target and restart of every call: the one graph
    ce1 = cpu(eng.apgd_attack(x, y, EPS, STEPS, trace=True))
    third = cpu(eng.apgdt_attack(x, y, EPS, **kw))
    ce2 = cpu(eng.apgd_attack(x, y, EPS, STEPS, trace=True))
    assert same(r, again) == [] and same(r, third) == [] and same(ce1, ce2) == []
    os.environ["VITLORA_NO_GRAPH"] = "1"
    try:
        eng2 = make_engine(c["cfg"], c["w"], c["lora"], precision=prec)
        eager = cpu(eng2.apgdt_attack(x, y, EPS, **kw))
        ce_eager = cpu(eng2.apgd_attack(x, y, EPS, STEPS, trace=True))
        assert eng2.counter("graph_captures") == 0
    finally:
        os.environ.pop("VITLORA_NO_GRAPH")
    assert same(r, eager) == [] and same(ce1, ce_eager) == []


# ---- 7. scratch ----------------------------------------------------------------------------------------------------------------
def _scratch(eng, batch, n, k, guard=0, fill=0):
    nbytes = eng.apgdt_scratch_bytes(batch, n, k)
    buf = torch.full((nbytes + 2 * guard + 512,), fill, dtype=torch.uint8, device="cuda")
    base = (buf.data_ptr() + guard + 255) // 256 * 256
    return buf, base, nbytes


def test_results_do_not_depend_on_the_scratch_and_nothing_outside_it_is_written():
    c, eng = case(), engine("f16")
    x, y = c["x"].cuda(), c["y"].cuda()
    guard, outs = 1 << 20, []
    kw = dict(steps=STEPS, n_target_classes=N_TARGET, n_restarts=2, seed=3, trace=True)
    for fill in (0x00, 0xFF):
        buf, base, nbytes = _scratch(eng, 8, STEPS, N_TARGET, guard=guard, fill=0xA5)
        off = base - buf.data_ptr()
        buf[off:off + nbytes] = fill
        outs.append(cpu(eng.apgdt_attack(x, y, EPS, scratch=(base, nbytes), **kw)))
        assert bool((buf[:off] == 0xA5).all()), "bytes BEFORE the scratch were written"
        assert bool((buf[off + nbytes:] == 0xA5).all()), "bytes AFTER the scratch were written"
    assert same(outs[0], outs[1]) == []
    assert not any(torch.isnan(v.float()).any() for v in outs[0].values())
    assert eng.apgdt_scratch_bytes(8, STEPS, N_TARGET) > eng.apgd_scratch_bytes(8, STEPS)
    E = pkg().VitLoraError
    with pytest.raises(E):                                      # one byte short
        eng.apgdt_attack(x, y, EPS, scratch=(base, nbytes - 1), **kw)
    small = eng.apgdt_scratch_bytes(8, STEPS, 1)                # (pieces are rounded to 256 bytes: 9 rows of 8 targets need two)
    assert small < eng.apgdt_scratch_bytes(8, STEPS, 9)
    with pytest.raises(E):                                      # sized for fewer targets
        eng.apgdt_attack(x, y, EPS, scratch=(base, small), steps=STEPS, n_target_classes=9)
    with pytest.raises(E):                                      # misaligned
        eng.apgdt_attack(x, y, EPS, scratch=(base + 64, nbytes), **kw)
    for bad in (dict(n_target_classes=c["cfg"].num_labels), dict(n_target_classes=0), dict(n_restarts=0)):
        with pytest.raises(E):
            eng.apgdt_attack(x, y, EPS, steps=STEPS, **{**dict(n_target_classes=N_TARGET), **bad})
    with pytest.raises(E):
        eng.apgdt_attack(x, y, float("nan"), steps=STEPS, n_target_classes=N_TARGET)
    with pytest.raises(E):
        eng.apgdt_attack(x, y, EPS, steps=STEPS, n_target_classes=N_TARGET, rho=1.5)
    torch.cuda.synchronize()
    del buf


def test_three_classes_are_refused():
    cfg, w, lora, x, y = make_case(batch=2, seed=5, num_labels=3)
    eng = make_engine(cfg, w, lora)
    with pytest.raises(pkg().VitLoraError, match="num_labels >= 4"):
        eng.apgdt_attack(x.cuda(), y.cuda(), EPS, steps=2, n_target_classes=2)


# ---- 8. facade ---------------------------------------------------------------------------------------------------------------------
def _model(prec="f16"):
    P, c = pkg(), case()
    cfg = c["cfg"]
    arch = P.ArchConfig(image_size=cfg.image_size, patch_size=cfg.patch_size, hidden=cfg.hidden, layers=cfg.layers,
                        heads=cfg.heads, mlp=cfg.mlp, num_labels=cfg.num_labels, ln_eps=cfg.ln_eps)
    m = P.create_vit_model(cfg.num_labels, arch=arch, precision=prec)
    m.load_state_dict(c["w"])
    return m.eval()


def test_apgdt_facade_and_run_suite():
    P, c = pkg(), case()
    model = _model()
    eng = model._engine()
    mean, std = P.get_normalization(None)
    x = c["x"].cuda()
    clean = eng.forward(x, normalise=True).argmax(1)
    y = clean.clone()
    y[0] = (y[0] + 1) % c["cfg"].num_labels                    # image 0 is clean-wrong
    with pytest.raises(ValueError):
        P.APGDT(model, norm="L2")
    with pytest.raises(ValueError):
        P.APGDT(model, eot_iter=2)
    assert P.APGDT(model, n_classes=4).n_target_classes == 3 and P.APGDT(model, n_classes=100).n_target_classes == 9
    # the normalisation sandwich equals the engine composition by hand
    xn = O.normalise(c["x"]).cuda()
    atk = P.APGDT(P.LogitsModel(model), norm="Linf", eps=EPS, steps=5, n_restarts=2, seed=7, n_classes=4)
    atk.set_normalization_used(mean=mean, std=std)
    got = atk(xn, y)
    eng.set_normalization(mean, std)
    x01 = eng.channel_affine(xn, std, mean)
    res = eng.apgdt_attack(x01, y, EPS, steps=5, n_target_classes=3, n_restarts=2, seed=7)
    want = eng.channel_affine(res["x_adv"], [1 / s for s in std], [-m / s for m, s in zip(mean, std)])
    assert torch.equal(got, want)
    assert torch.equal(atk.last["x_adv"], res["x_adv"]) and (~res["robust"]).any()
    # run_suite: APGD-T's point only for the images APGD-CE left robust
    eps = EPS / 8                                               # small enough that APGD-CE with 5 steps leaves images robust
    kw = dict(bs=8, seed=1, steps=5, n_target_classes=3, square_queries=30)
    o1, ra1 = P.run_suite(model, x, y, eps, attacks=["apgd-ce"], **kw)
    o2, ra2 = P.run_suite(model, x, y, eps, attacks=["apgd-ce", "apgd-t"], **kw)
    ot, rat = P.run_suite(model, x, y, eps, attacks=["apgd-t"], **kw)
    fooled1 = (o1 != x).flatten(1).any(1)
    assert torch.equal(o2[fooled1], o1[fooled1])                # never moves an image APGD-CE fooled
    assert torch.equal(o2[~fooled1], ot[~fooled1])              # the others are APGD-T's (x itself where it fooled nothing)
    assert ra2 <= ra1
    print(f"robust accuracy at eps {eps:.5f}: apgd-ce {ra1}, apgd-ce + apgd-t {ra2}, apgd-t {rat}")
    for o, ra in ((o1, ra1), (o2, ra2), (ot, rat)):
        pred = eng.forward(o, normalise=True).argmax(1)
        changed = (o != x).flatten(1).any(1)
        assert not changed[0] and (pred != y)[changed].all() and (pred == y)[~changed][1:].all()
        assert (o - x).abs().max().item() <= eps + 1e-7
        assert ra == float((~changed)[1:].sum()) / 8
    # run_suite is what AutoAttack runs
    o3, ra3 = P.run_suite(model, x, y, eps, attacks=["apgd-ce", "square"], **kw)
    aa = P.AutoAttack(model, norm="Linf", eps=eps, version="custom", attacks_to_run=["apgd-ce", "square"], seed=1, steps=5,
                      square_queries=30)
    assert torch.equal(aa.run_standard_evaluation(x, y, bs=8), o3) and aa.robust_accuracy == ra3
    with pytest.raises(NotImplementedError):
        P.run_suite(model, x, y, eps, attacks=["apgd-ce", "fab-t"])
    with pytest.raises(ValueError):
        P.run_suite(model, x, y, eps, attacks=[])


def test_auto_attack_cli_runs_the_three_components(tmp_path, capsys):
    import sys
    from helpers import ROOT
    sys.path.insert(0, ROOT)
    auto_attack = importlib.import_module("auto_attack")
    out = tmp_path / "adv"
    auto_attack.main(["--model", "google_vit", "--source", "gtsrb", "--output_dir", str(out), "--synthetic", "8", "--arch", "tiny",
                      "--num_classes", "10", "--batch_size", "8", "--steps", "3", "--splits", "val", "--attacks", "apgd-ce", "apgd-t",
                      "square", "--square_queries", "10", "--n_target_classes", "20"])
    text = capsys.readouterr().out
    assert "robust accuracy under apgd-ce + apgd-t + square (eps 0.031, 3 steps, 9 targets × 3 steps, 10 queries): " in text
    assert sorted(os.listdir(out / "google_vit" / "gtsrb" / "val" / "auto" / "images")) == [f"val_{i:06d}.png" for i in range(8)]


# ---- 9. one full-size case -----------------------------------------------------------------------------------------------------
def test_vit_b16_batch3():
    P = pkg()
    syn = importlib.import_module(PKG + ".synthetic")
    targets = ("q", "k", "v", "o", "fc2")
    arch = P.ArchConfig(num_labels=21)
    eng = P.Engine(arch, P.LoraSpec(r=8, alpha=16.0, dropout=0.0, targets=targets))
    eng.load_state_dict(syn.random_state_dict(arch, seed=0))
    for (i, t), (A_, B_) in syn.random_lora(arch, 8, targets, seed=1).items():
        eng.param(i, t, "A").copy_(A_)
        eng.param(i, t, "B").copy_(B_)
    x, _ = syn.random_batch(arch, 3, seed=100)
    y = eng.forward(x.cuda(), normalise=True).argmax(1).cpu()
    y[0] = (y[0] + 1) % 21
    r = cpu(eng.apgdt_attack(x.cuda(), y.cuda(), 8 / 255, steps=2, n_target_classes=2, trace=True))
    eng.check()                                                 # no error word
    check_result(eng, r, x, y, 8 / 255, 2)
    assert torch.isfinite(r["loss_best"]).all() and torch.isfinite(r["trace_loss"]).all()
