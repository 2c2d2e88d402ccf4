"""GPU tests of Auto-PGD (APGD-CE, L-inf): vl_apgd_step, vl_debug_apgd_track, vl_apgd_attack and the APGD / AutoAttack facade.

The reference is tests/apgd_ref.py, a numpy float32 restatement of the algorithm text.  The two kernels
are held to it bit for bit on caller-made inputs; the whole attack is held to it through its OWN trace (the bookkeeping must be
what the state machine makes of the losses and predictions the GPU saw) -- full-trajectory parity with the CPU oracle is
deliberately not asked: the oracle's own decision margins fall to 4e-7 by N = 25 on this case, so any rounding difference in the
forward changes the path.  Tolerances: TOL_ACT as in tests/test_hip_engine.py (f16 4e-3, f32 1e-4) and, for bf16, the 1.5e-2 that
tests/test_hip_bf16.py holds logits and loss to."""
import importlib
import os

import numpy as np
import pytest
import torch

import apgd_ref as R
from helpers import O, make_case, make_engine, pkg

pytestmark = pytest.mark.gpu

F32 = np.float32
PRECS = ["f16", "bf16", "f32"]
TOL_ACT = {"f16": 4e-3, "f32": 1e-4, "bf16": 1.5e-2}
EPS = 0.5 / 255


# ---- shared case: make_case(batch=8, seed=5), labels = the clean argmax of the CPU oracle ---------------------------------------
_CASE, _ENG, _RUN = {}, {}, {}


def case():
    if not _CASE:
        cfg, w, lora, x, _ = make_case(batch=8, seed=5)
        y = O.vit_forward(w, cfg, O.normalise(x), lora).argmax(1)
        _CASE.update(cfg=cfg, w=w, lora=lora, x=x, y=y)
    return _CASE


def engine(prec):
    if prec not in _ENG:
        c = case()
        _ENG[prec] = make_engine(c["cfg"], c["w"], c["lora"], precision=prec)
    return _ENG[prec]


def run(prec, n, **kw):
    """One traced attack from x on the shared case (computed once per key, never modified)."""
    key = (prec, n, tuple(sorted(kw.items())))
    if key not in _RUN:
        c = case()
        r = engine(prec).apgd_attack(c["x"].cuda(), c["y"].cuda(), EPS, n, trace=True, **kw)
        torch.cuda.synchronize()
        _RUN[key] = {k: v.cpu() for k, v in r.items()}
    return _RUN[key]


def per_image_ce(eng, x, y):
    """Forward + CE of the library at the batch size of x: the per-image losses the attack's track kernel reads."""
    logits = eng.forward(x, normalise=True).clone()
    eng.loss_ce(y)
    loss = eng.debug_tensor("loss_img", 0)[:x.shape[0]].clone()
    torch.cuda.synchronize()
    return loss.cpu(), logits.cpu()


# ---- 1. the step kernel, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("a", [1.0, 0.75])
@pytest.mark.parametrize("side", [16, 64])
def test_apgd_step_kernel_bit_exact(side, a, last):
    """B = 8 images carrying all eight flag combinations, per-image step sizes 2 eps / eps / eps / 4, zeros planted in the
    gradients; 3 x 16 x 16 is less than one block's stride (192 vectors for 256 threads), 3 x 64 x 64 takes several blocks."""
    g = torch.Generator().manual_seed(side + int(a * 100) + int(last))
    shape = (8, 3, side, side)
    eps = 8 / 255
    x0 = torch.rand(shape, generator=g)
    near = lambda: (x0 + (torch.rand(shape, generator=g) * 2 - 1) * eps).clamp(0, 1)        # noqa: E731
    x_adv, x_old, x_best, x_best_adv = near(), near(), near(), near()
    grad, grad_best = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    for t in (grad, grad_best):
        t.view(-1)[::7] = 0.0
        t.view(-1)[1::11] = 1e-30
        t.view(-1)[2::13] = -1e-38
    flags = torch.arange(8, dtype=torch.int32)
    step = torch.tensor([2 * eps, eps, eps / 4, 2 * eps, eps, eps / 4, 2 * eps, eps], dtype=torch.float32)
    want = R.step(x_adv.numpy(), x_old.numpy(), x_best.numpy(), x_best_adv.numpy(), grad_best.numpy(), x0.numpy(), grad.numpy(),
                  flags.numpy(), step.numpy(), eps, a, last)
    dev = [t.cuda().contiguous() for t in (x_adv, x_old, x_best, x_best_adv, grad_best, x0, grad, flags, step)]
    engine("f16").apgd_step(*dev, eps, a, last)
    torch.cuda.synchronize()
    for name, got, ref in zip(("x_adv", "x_old", "x_best", "x_best_adv", "grad_best"), dev[:5], want):
        assert np.array_equal(got.cpu().numpy(), ref), (name, int((got.cpu().numpy() != ref).sum()))
    assert torch.equal(dev[5].cpu(), x0) and torch.equal(dev[6].cpu(), grad)               # inputs are not written
    if not last:
        assert (dev[0].cpu() - x0).abs().max().item() <= eps + 1e-7


def test_apgd_step_refuses_shapes_the_kernel_cannot_run():
    eng = engine("f16")
    t = [torch.zeros(2, 6, device="cuda") for _ in range(7)] + [torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, device="cuda")]
    with pytest.raises(pkg().VitLoraError):
        eng.apgd_step(*t, 0.1, 1.0)                      # 6 floats per image: not a multiple of 4


# ---- 2. the track kernel, exactly ------------------------------------------------------------------------------------------------
def _scratch(eng, batch, n, guard=0, fill=0):
    nbytes = eng.apgd_scratch_bytes(batch, n)
    buf = torch.full((nbytes + 2 * guard + 512,), fill, dtype=torch.uint8, device="cuda")
    base = (buf.data_ptr() + guard + 255) // 256 * 256
    return buf, base, nbytes


@pytest.mark.parametrize("n", [10, 25, 100])
def test_apgd_track_kernel_matches_the_state_machine(n):
    """Synthetic loss rows (increasing, constant, saw-tooth, ties, rise-drop-rise, random) and prediction rows; logits rows whose
    argmax is or is not the label, with tied maxima on either side of it.  Every call's step, flag word, loss_best and robust
    equal the reference's."""
    eng = engine("f16")
    cls = case()["cfg"].num_labels
    rng = np.random.default_rng(n)
    j = np.arange(n + 1, dtype=F32)
    rows = [1 + j, np.ones(n + 1, F32), 1 + (j % 3), np.repeat(np.arange((n + 2) // 2, dtype=F32), 2)[:n + 1] + 1,
            np.where(j < n // 4 + 1, 1 + j, 0.1 + 0.001 * j), rng.random(n + 1).astype(F32), 2 - 0.01 * j,
            np.round(rng.random(n + 1) * 4).astype(F32) / 4]
    losses = np.stack(rows, 1).astype(F32)                         # [n + 1, B]
    B = losses.shape[1]
    preds = np.ones((n + 1, B), bool)
    preds[n // 2, 1] = False
    preds[:, 2] = rng.random(n + 1) > 0.3
    preds[0, 3] = False
    preds[n, 4] = False
    preds[:, 5] = rng.random(n + 1) > 0.7
    labels = torch.tensor([3, 0, 9, 5, 1, 7, 2, 4], dtype=torch.int64)
    eng.plan(B)
    buf, base, nbytes = _scratch(eng, B, n, fill=0xFF)
    sm = R.StateMachine(B, n, EPS)
    for it in range(n + 1):
        logits = rng.standard_normal((B, cls)).astype(F32)
        for b in range(B):
            y = int(labels[b])
            other = (y + 1 + it % (cls - 1)) % cls
            logits[b, y if preds[it, b] else other] = 5.0
            if it % 4 == 1:                # a tied maximum: argmax is the FIRST one, so the label wins only from the lower index
                lo, hi = min(y, other), max(y, other)
                logits[b, lo] = logits[b, hi] = 5.0
                preds[it, b] = lo == y
        want_flags = sm.start(losses[it], preds[it]) if it == 0 else sm.observe(it - 1, losses[it], preds[it])
        step, flags, best, robust = eng.apgd_track((base, nbytes), B, n, EPS, 0.75, torch.from_numpy(losses[it]).cuda(),
                                                   torch.from_numpy(logits).cuda(), labels.cuda(), reset=it == 0)
        torch.cuda.synchronize()
        assert np.array_equal(flags.cpu().numpy(), want_flags), (it, flags.cpu().tolist(), want_flags.tolist())
        assert np.array_equal(step.cpu().numpy(), sm.step), it
        assert np.array_equal(best.cpu().numpy(), sm.loss_best), it
        assert np.array_equal(robust.cpu().numpy() != 0, sm.robust), it


# ---- 3. trace consistency --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [10, 25])
@pytest.mark.parametrize("prec", PRECS)
def test_attack_bookkeeping_is_the_state_machine_on_its_own_trace(prec, n):
    r = run(prec, n)
    step, _, best, robust = R.replay(r["trace_loss"].numpy(), r["trace_pred"].numpy(), EPS)
    assert np.array_equal(r["trace_step"].numpy(), step)
    assert np.array_equal(r["loss_best"].numpy(), best)
    assert np.array_equal(r["robust"].numpy(), robust)
    if prec == "f32":
        assert r["trace_pred"][0].all()                    # labels are the CPU oracle's clean argmax: the fp32 path agrees with it


# ---- 4. invariants ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [10, 25])
@pytest.mark.parametrize("prec", PRECS)
def test_attack_invariants(prec, n):
    c, r, eng = case(), run(prec, n), engine(prec)
    x, y = c["x"], c["y"]
    for k in ("x_best", "x_best_adv"):
        assert (r[k] - x).abs().max().item() <= EPS + 1e-6, k
        assert r[k].min().item() >= 0 and r[k].max().item() <= 1, k
    assert (r["loss_best"] >= r["trace_loss"][0]).all()
    assert torch.equal(r["loss_best"], r["trace_loss"].max(0).values)
    # x_best carries loss_best: re-forwarded at the same batch size
    loss, _ = per_image_ce(eng, r["x_best"].cuda(), y.cuda())
    err = (loss - r["loss_best"]).abs() / r["loss_best"].abs().clamp_min(1.0)
    print(f"{prec} N={n}: re-forwarded x_best CE differs from loss_best by at most {err.max().item():.3e} (bit-equal: {torch.equal(loss, r['loss_best'])})")
    assert err.max().item() < TOL_ACT[prec]
    # every image reported as not robust is misclassified at x_best_adv
    _, logits = per_image_ce(eng, r["x_best_adv"].cuda(), y.cuda())
    fooled = ~r["robust"]
    assert (logits.argmax(1) != y)[fooled].all()
    print(f"{prec} N={n}: robust = {r['robust'].int().tolist()}")
    if prec == "f32":        # the CPU reference ends this case with [1,0,0,1,0,0,0,1] (smallest logit margin 4.8e-2): both outcomes
        assert r["robust"].any() and fooled.any()


# ---- 5. one step from x is the FGSM point ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_one_step_from_x_equals_one_pgd_step_with_alpha_eps(prec):
    c, r, eng = case(), run(prec, 1), engine(prec)
    pgd = eng.pgd_attack(c["x"].cuda(), c["y"].cuda(), EPS, EPS, 1, random_start=False).cpu()
    improved = r["trace_loss"][1] > r["trace_loss"][0]
    assert improved.any()
    assert (r["x_best"] - pgd)[improved].abs().max().item() <= 1e-6
    assert torch.equal(r["x_best"][~improved], c["x"][~improved])


# ---- 6. graph replay == eager ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_graph_replay_equals_eager_and_the_graph_is_reused(prec):
    c, r = case(), run(prec, 10)
    eng = engine(prec)
    eng.apgd_attack(c["x"].cuda(), c["y"].cuda(), EPS, 10)       # (the engine keeps two scratch tensors: make this key current)
    before = eng.counter("graph_captures")
    again = eng.apgd_attack(c["x"].cuda(), c["y"].cuda(), EPS, 10, trace=True)
    assert eng.counter("graph_captures") == before           # same (batch, eps, steps, scratch, rho): nothing new is captured
    os.environ["VITLORA_NO_GRAPH"] = "1"
    try:
        eng2 = make_engine(c["cfg"], c["w"], c["lora"], precision=prec)
        eager = eng2.apgd_attack(c["x"].cuda(), c["y"].cuda(), EPS, 10, trace=True)
        assert eng2.counter("graph_captures") == 0
    finally:
        os.environ.pop("VITLORA_NO_GRAPH")
    for k, v in r.items():
        assert torch.equal(v, again[k].cpu()), ("second call", k)
        assert torch.equal(v, eager[k].cpu()), ("eager", k)
    # another step count is another graph, and dropping the graphs (a switch changed) captures again
    eng.apgd_attack(c["x"].cuda(), c["y"].cuda(), EPS, 3)
    assert eng.counter("graph_captures") == before + 1
    eng.set_option("fuse_pgd", 1)
    eng.apgd_attack(c["x"].cuda(), c["y"].cuda(), EPS, 10)
    assert eng.counter("graph_captures") == before + 2


def test_attack_under_the_lds_poison_hook_runs_eagerly_and_equals_the_replay():
    """"poison_lds" (process-wide) takes the attack off the graph, as it does vl_pgd_attack: every launch is preceded by a kernel
    that fills LDS with NaN patterns.  The APGD kernels keep nothing in LDS between launches, so nothing may change."""
    c, r, eng = case(), run("f16", 10), engine("f16")
    n0, g0 = eng.counter("lds_poisons"), eng.counter("graph_captures")
    try:
        eng.set_option("poison_lds", 1)
        got = eng.apgd_attack(c["x"].cuda(), c["y"].cuda(), EPS, 10, trace=True)
        torch.cuda.synchronize()
    finally:
        eng.set_option("poison_lds", 0)
    assert eng.counter("lds_poisons") - n0 > 100 and eng.counter("graph_captures") == g0
    for k, v in r.items():
        assert torch.equal(v, got[k].cpu()), k


# ---- 7. repeatability, scratch contents, guard band ------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_results_do_not_depend_on_the_scratch_and_nothing_outside_it_is_written(prec):
    c, eng = case(), engine(prec)
    n, guard = 10, 1 << 20
    outs = []
    for fill in (0x00, 0xFF):
        buf, base, nbytes = _scratch(eng, 8, n, guard=guard, fill=0xA5)
        off = base - buf.data_ptr()
        buf[off:off + nbytes] = fill
        for _ in range(2):
            r = eng.apgd_attack(c["x"].cuda(), c["y"].cuda(), EPS, n, random_start=True, seed=3, trace=True, scratch=(base, nbytes))
            torch.cuda.synchronize()
            outs.append({k: v.cpu() for k, v in r.items()})
        assert bool((buf[:off] == 0xA5).all()), "bytes BEFORE the scratch were written"
        assert bool((buf[off + nbytes:] == 0xA5).all()), "bytes AFTER the scratch were written"
    for o in outs[1:]:
        for k, v in outs[0].items():
            assert not torch.isnan(o[k].float()).any(), k
            assert torch.equal(v, o[k]), k
    other = eng.apgd_attack(c["x"].cuda(), c["y"].cuda(), EPS, n, random_start=True, seed=4, trace=True)
    assert not torch.equal(other["trace_loss"][0].cpu(), outs[0]["trace_loss"][0])
    with pytest.raises(pkg().VitLoraError):                  # a scratch one byte short is refused, nothing runs
        eng.apgd_attack(c["x"].cuda(), c["y"].cuda(), EPS, n, scratch=(base, nbytes - 1))


# ---- 8. the start point ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_x_init_and_the_random_start(prec):
    c, eng = case(), engine(prec)
    x, y = c["x"], c["y"]
    g = torch.Generator().manual_seed(11)
    x_init = x + (torch.rand(x.shape, generator=g) * 2 - 1) * EPS            # not clamped: the library clamps to [0,1]
    r = eng.apgd_attack(x.cuda(), y.cuda(), EPS, 3, x_init=x_init.cuda(), trace=True)
    first = r["trace_loss"][0].cpu()
    loss, _ = per_image_ce(eng, x_init.clamp(0, 1).cuda(), y.cuda())
    assert torch.equal(first, loss)
    assert not torch.equal(first, run(prec, 1)["trace_loss"][0])             # and it is not the loss at x
    if prec == "f32":
        ref, _, _, _ = R.eval_point(c["w"], c["cfg"], x_init.clamp(0, 1), y, c["lora"])
        err = np.abs(first.numpy() - ref) / np.maximum(1.0, np.abs(ref))
        assert err.max() < TOL_ACT["f32"], err.max()
    # random start: an image that is never fooled keeps the start point in x_best_adv
    r = eng.apgd_attack(x.cuda(), y.cuda(), 2 * EPS / 100, 1, random_start=True, seed=9)
    keep = r["robust"].cpu()
    assert keep.any()
    d = (r["x_best_adv"].cpu() - x)[keep]
    assert d.abs().max().item() <= 2 * EPS / 100 + 1e-7
    assert d.abs().amax(dim=(1, 2, 3)).min().item() > 0.9 * 2 * EPS / 100      # t / max|t| reaches the ball's surface in every image
    assert abs(d.mean().item()) < 0.05 * 2 * EPS / 100


# ---- 9. facade -------------------------------------------------------------------------------------------------------------------
def _model(prec="f16"):
    P, c = pkg(), case()
    cfg = c["cfg"]
    arch = P.ArchConfig(image_size=cfg.image_size, patch_size=cfg.patch_size, hidden=cfg.hidden, layers=cfg.layers,
                        heads=cfg.heads, mlp=cfg.mlp, num_labels=cfg.num_labels, ln_eps=cfg.ln_eps)
    m = P.create_vit_model(cfg.num_labels, arch=arch, precision=prec)
    m.load_state_dict(c["w"])
    return m.eval()


def test_autoattack_facade():
    P, c = pkg(), case()
    model = _model()
    x = c["x"].cuda()
    with pytest.raises(NotImplementedError, match="APGD-T, FAB-T and Square"):
        P.AutoAttack(model, norm="Linf", eps=EPS, version="standard")
    with pytest.raises(ValueError):
        P.APGD(model, norm="L2")
    with pytest.raises(ValueError):
        P.APGD(model, loss="dlr")
    eng = model._engine()
    clean = eng.forward(x, normalise=True).argmax(1).cpu()
    y = clean.clone()
    y[0] = (y[0] + 1) % c["cfg"].num_labels               # image 0 is clean-wrong
    adv = P.AutoAttack(model, norm="Linf", eps=EPS, version="custom", attacks_to_run=["apgd-ce"], seed=1, steps=10)
    out = adv.run_standard_evaluation(x, y.cuda(), bs=8).cpu()
    pred = eng.forward(out.cuda(), normalise=True).argmax(1).cpu()
    changed = (out != c["x"]).flatten(1).any(1)
    assert not changed[0]                                  # clean-wrong: returned as it was
    assert (pred != y)[changed].all()                      # what was replaced is misclassified
    assert (pred == y)[~changed][1:].all()                 # still robust: bit-equal to x and still right
    assert changed.any()
    assert (out - c["x"]).abs().max().item() <= EPS + 1e-6
    assert adv.robust_accuracy == float((~changed)[1:].sum()) / 8
    # two batches of 4 give what one batch of 8 gives for the images that stay as they were
    out2 = adv.run_standard_evaluation(x, y.cuda(), bs=4).cpu()
    assert not (out2[0] != c["x"][0]).any()


def test_apgd_normalisation_sandwich_matches_pgds():
    """set_normalization_used(mean, std): the inputs ARE normalised; they are mapped back to [0,1], attacked there with the model
    fed normalised pixels, and the result is normalised again -- the same sandwich as PGD (attacks._Attack)."""
    P, c = pkg(), case()
    model = _model()
    eng = model._engine()
    mean, std = P.get_normalization(None)
    y = c["y"].cuda()
    xn = O.normalise(c["x"]).cuda()
    atk = P.APGD(P.LogitsModel(model), norm="Linf", eps=4 * EPS, steps=5, n_restarts=2, seed=7)
    atk.set_normalization_used(mean=mean, std=std)
    got = atk(xn, y)
    # by hand
    eng.set_normalization(mean, std)
    x = eng.channel_affine(xn, std, mean)
    correct = eng.forward(x, normalise=True).argmax(1) == y
    want, robust = x.clone(), correct.clone()
    for r in range(2):
        res = eng.apgd_attack(x, y, 4 * EPS, 5, random_start=True, seed=7 + r)
        take = robust & ~res["robust"]
        want[take] = res["x_best_adv"][take]
        robust &= res["robust"]
    want = eng.channel_affine(want, [1 / s for s in std], [-m / s for m, s in zip(mean, std)])
    assert torch.equal(got, want)
    assert (~robust).any()
    # PGD through the same sandwich moves the same kind of pixels: inside the eps-ball of the [0,1] image
    pgd = P.PGD(P.LogitsModel(model), eps=4 * EPS, alpha=EPS, steps=5, random_start=False)
    pgd.set_normalization_used(mean=mean, std=std)
    st = torch.tensor(std).view(1, 3, 1, 1).cuda()
    for adv in (got, pgd(xn, y)):
        assert ((adv - xn) * st).abs().max().item() <= 4 * EPS + 1e-5


def test_auto_attack_cli_writes_the_reference_layout(tmp_path):
    import sys
    from helpers import ROOT
    sys.path.insert(0, ROOT)
    auto_attack = importlib.import_module("auto_attack")
    out = tmp_path / "adv"
    auto_attack.main(["--model", "google_vit", "--source", "gtsrb", "--output_dir", str(out), "--synthetic", "8", "--arch", "tiny",
                      "--num_classes", "10", "--batch_size", "8", "--steps", "5", "--splits", "val", "test"])
    from PIL import Image
    for split in ("val", "test"):
        d = out / "google_vit" / "gtsrb" / split / "auto" / "images"
        names = sorted(os.listdir(d))
        assert names == [f"{split}_{i:06d}.png" for i in range(8)]
        img = Image.open(d / names[0])
        assert img.size == (64, 64) and img.mode == "RGB"
