"""CPU tests of the APGD-T reference restatement (tests/apgdt_ref.py): the DLR-targeted loss and its scaled gradient against torch
autograd of the formula, the float32 restatement against the float64 one, the target picker against the package's torch.sort
construction, and the whole reference attack on the shared tiny case.  No GPU.  The GPU tests
(tests/test_hip_apgdt.py) hold the kernels to the same reference and run the same whole-attack case."""
import numpy as np
import pytest
import torch

import apgdt_ref as R
from helpers import O, make_case

CLASSES = [4, 5, 10, 21, 70]
ROWS = 64
EPS, STEPS, N_TARGET = R.CASE_EPS, R.CASE_STEPS, R.CASE_N_TARGET      # test_reference_attack_on_the_shared_case records what they give


def rows(C, seed=0):
    """ROWS rows of standard-normal logits that are float32 numbers (so both precisions read the same values), labels and
    targets at random ranks with target != label."""
    g = torch.Generator().manual_seed(1000 * C + seed)
    z = torch.randn(ROWS, C, generator=g).numpy().astype(np.float32)
    y = torch.randint(0, C, (ROWS,), generator=g).numpy()
    t = (y + 1 + torch.randint(0, C - 1, (ROWS,), generator=g).numpy()) % C
    return z, y, t


@pytest.mark.parametrize("C", CLASSES)
def test_float64_loss_and_gradient_equal_autograd_of_the_formula(C):
    z, y, t = rows(C)
    loss, grad = R.dlr_targeted(z, y, t, np.float64)
    zt = torch.from_numpy(z.astype(np.float64)).requires_grad_(True)
    want = R.dlr_torch(zt, torch.from_numpy(y), torch.from_numpy(t))
    (g,) = torch.autograd.grad(want.sum(), zt)
    srt = torch.sort(zt.detach(), dim=1, descending=True).values
    D = srt[:, 0] - 0.5 * (srt[:, 2] + srt[:, 3]) + 1e-12
    err_l = np.abs(loss - want.detach().numpy()).max()
    err_g = np.abs(grad - (g * D[:, None]).numpy()).max()
    print(f"C={C}: loss err {err_l:.2e}, D * gradient err {err_g:.2e}, smallest D {float(D.min()):.3e}")
    assert err_l <= 1e-12 and err_g <= 1e-12


@pytest.mark.parametrize("C", CLASSES)
def test_float32_restatement_matches_float64_where_the_denominator_is_not_small(C):
    """Error model: z_pi3 + z_pi4 is rounded once (|sum| < 10: 3e-7 in its half), the two differences and the quotient once each
    (6e-8 relative); with D >= 0.1 that is below 4e-6 relative in q."""
    z, y, t = rows(C)
    l64, g64 = R.dlr_targeted(z, y, t, np.float64)
    l32, g32 = R.dlr_targeted(z, y, t, np.float32)
    assert l32.dtype == np.float32 and g32.dtype == np.float32
    srt = -np.sort(-z.astype(np.float64), axis=1)
    ok = (srt[:, 0] - 0.5 * (srt[:, 2] + srt[:, 3])) >= 0.1
    assert ok.sum() >= ROWS // 2                       # the generator leaves most rows in
    err_l = np.abs(l32[ok] - l64[ok]) / np.abs(l64[ok])
    err_g = np.abs(g32[ok] - g64[ok]).max(1) / np.abs(g64[ok]).max(1)
    print(f"C={C}: {int(ok.sum())} rows, loss rel err {err_l.max():.2e}, gradient rel err {err_g.max():.2e}")
    assert err_l.max() <= 1e-5 and err_g.max() <= 1e-5


@pytest.mark.parametrize("C", CLASSES)
def test_targets_equal_the_sort_construction_on_clean_correct_rows(C):
    z, _, _ = rows(C, seed=1)
    y = z.argmax(1)
    y[::5] = (y[::5] + 1) % C                          # every fifth row is clean-wrong
    n = min(9, C - 1)
    got = R.targets(z, y, n)
    idx = torch.sort(torch.from_numpy(z), dim=1).indices
    correct = z.argmax(1) == y
    assert correct.any() and (~correct).any()
    for k in range(n):
        assert np.array_equal(got[k][correct], idx[:, -(k + 2)].numpy()[correct]), k
    for b in range(ROWS):                              # every row: distinct classes, none the label, logits descending
        assert len(set(got[:, b])) == n and int(y[b]) not in got[:, b]
        assert (np.diff(z[b, got[:, b]]) <= 0).all()


def test_ties_go_to_the_lower_index_and_four_classes_give_three_targets():
    z = np.array([[1, 3, 3, 3, 0], [2, 2, 2, 2, 2], [0, -0.0, 5, 0, 1]], np.float32)
    y = np.array([1, 0, 2])
    assert R.targets(z, y, 4).T.tolist() == [[2, 3, 0, 4], [1, 2, 3, 4], [4, 0, 1, 3]]
    z4 = np.array([[0.5, 2, 2, -1], [7, 7, 7, 7]], np.float32)
    assert R.targets(z4, np.array([1, 3]), 3).T.tolist() == [[2, 0, 3], [0, 1, 2]]
    # the loss ranks the same way: with the four largest logits equal D is 1e-12 and everything stays finite
    loss, grad = R.dlr_targeted(z4[1:], np.array([3]), np.array([0]), np.float32)
    assert np.isfinite(loss).all() and np.isfinite(grad).all() and loss[0] == 0
    assert grad[0].tolist() == [1, 0, 0, -1]


_S = {}


def shared_case():
    """make_case(batch=8, seed=5), labels = the oracle's clean argmax, image 0's label changed (clean-wrong)."""
    if not _S:
        cfg, w, lora, x, _ = make_case(batch=8, seed=5)
        y = O.vit_forward(w, cfg, O.normalise(x), lora).argmax(1)
        y[0] = (y[0] + 1) % cfg.num_labels
        _S.update(cfg=cfg, w=w, lora=lora, x=x, y=y)
    return _S


def test_reference_attack_on_the_shared_case():
    """EPS = 0.5 / 255, STEPS = 10, N_TARGET = 3, one restart, seed 0: the reference fools 5 of the 7 clean-correct images (all in
    run 0, the most likely wrong class) and leaves 2 robust."""
    c = shared_case()
    x, y = c["x"], c["y"]
    r = R.attack(c["w"], c["cfg"], x.numpy(), y, EPS, STEPS, N_TARGET, 1, lora=c["lora"])
    changed = (r["x_adv"] != x.numpy()).reshape(8, -1).any(1)
    print(f"fooled {int(changed.sum())}, robust {int(r['robust'].sum())}, fooled_by {r['fooled_by'].tolist()}")
    assert not r["clean_correct"][0] and r["clean_correct"][1:].all()
    assert changed.sum() >= 1 and r["robust"].sum() >= 1
    pred = O.vit_forward(c["w"], c["cfg"], O.normalise(torch.from_numpy(r["x_adv"])), c["lora"]).argmax(1)
    assert (pred != y).numpy()[changed].all()                         # every replaced image is misclassified by the oracle
    assert np.abs(r["x_adv"] - x.numpy()).max() <= EPS + 1e-7
    assert not changed[0]                                              # the clean-wrong image is untouched
    assert np.array_equal(changed, r["fooled_by"] >= 0)
    assert np.array_equal(r["robust"], r["clean_correct"] & r["robust_run"].all(0))
    assert np.array_equal(r["x_adv"][~changed], x.numpy()[~changed])   # untouched images equal x
    assert r["targets"].shape == (N_TARGET, 8) and (r["targets"] != y.numpy()[None]).all()
