"""CPU-only tests of the Auto-PGD restatement (tests/apgd_ref.py) and of the package's schedule helper: known answers that follow
from the algorithm text alone.  The GPU tests (tests/test_hip_apgd.py) hold the kernels to this file's
subject."""
import numpy as np
import torch

import apgd_ref as R
from helpers import O, make_case, pkg

F32 = np.float32
SCHED_100 = [(21, 22), (40, 19), (56, 16), (69, 13), (79, 10), (86, 7), (92, 6), (98, 6)]
SCHED_10 = [(1, 2)] + [(i, 1) for i in range(2, 10)]
# N = 25: k0 = int(5.5) = 5, k_min = int(1.5) = 1, dec = max(int(.75), 1) = 1
SCHED_25 = [(4, 5), (8, 4), (11, 3), (13, 2)] + [(i, 1) for i in range(14, 25)]


def test_apgd_schedule_known_answers():
    P = pkg()
    for n, want in ((100, SCHED_100), (10, SCHED_10), (25, SCHED_25)):
        assert P.apgd_schedule(n) == want, n
        assert R.schedule(n) == want, n
    assert P.apgd_schedule(1) == [(0, 1)]


def _steps(losses, preds=None, eps=8 / 255, rho=.75):
    losses = np.asarray(losses, F32).reshape(len(losses), -1)
    preds = np.ones_like(losses, bool) if preds is None else np.asarray(preds, bool).reshape(losses.shape)
    return R.replay(losses, preds, eps, rho)


def test_constant_positive_loss_halves_the_step_at_every_checkpoint():
    for n, sched in ((100, SCHED_100), (10, SCHED_10), (25, SCHED_25)):
        step, flags, best, robust = _steps(np.ones(n + 1))
        want = F32(2) * F32(8 / 255)
        ck = {i for i, _ in sched}
        for i in range(n):
            assert step[i, 0] == want, (n, i)          # the step iteration i's update uses
            assert bool(flags[i + 1, 0] & R.RESTART) == (i in ck)
            if i in ck:
                want = want / F32(2)
        assert best[0] == 1 and robust[0]
        assert flags[0, 0] == (R.IMPROVED | R.FOOLED) and not (flags[1:, 0] & R.IMPROVED).any()


def test_strictly_increasing_loss_never_halves_the_step():
    for n in (100, 10, 25):
        step, flags, best, _ = _steps(np.arange(1, n + 2))
        assert (step == F32(2) * F32(8 / 255)).all()
        assert not (flags & R.RESTART).any()
        assert (flags[1:, 0] & R.IMPROVED).all() and best[0] == n + 1


def test_a_flat_spell_after_a_no_reduce_check_triggers_noimp():
    """N = 100: rising up to the first checkpoint (i = 21: no reduction, reduced_last = 0); then the loss drops and climbs again
    without reaching the best -- 18 of the 19 comparisons of the second window rise (no oscillation) but loss_best did not move."""
    n = 100
    losses = np.zeros(n + 1, F32)
    losses[0] = 0.5
    losses[1:23] = np.arange(1, 23)                       # loss_steps[0 .. 21] = 1 .. 22
    losses[23:] = 0.1 + 0.001 * np.arange(n + 1 - 23)     # loss_steps[22 ..]: far below the best, strictly rising
    step, flags, best, _ = _steps(losses)
    assert not flags[22, 0] & R.RESTART                   # checkpoint i = 21
    assert flags[41, 0] & R.RESTART                       # checkpoint i = 40: noimp
    assert step[40, 0] == F32(2) * F32(8 / 255) and step[41, 0] == F32(8 / 255)
    assert best[0] == 22
    # the check after a reduction cannot fire on noimp (reduced_last = 1), and the window still rises: no reduction at i = 56
    assert not flags[57, 0] & R.RESTART


def test_robust_and_fooled_flags_follow_pred():
    preds = np.ones((11, 2), bool)
    preds[4, 1] = False
    step, flags, _, robust = R.replay(np.tile(np.arange(1, 12, dtype=F32)[:, None], (1, 2)), preds, 0.1)
    assert robust.tolist() == [True, False]
    assert [bool(f & R.FOOLED) for f in flags[1:, 1]] == [i == 3 for i in range(10)]
    assert not (flags[1:, 0] & R.FOOLED).any()


def test_the_restart_takes_x_best_and_leaves_x_old_alone():
    eps, st, a = F32(0.25), F32(0.125), F32(.75)
    x0 = np.full((1, 4), 0.5, F32)
    x_adv = np.array([[0.60, 0.40, 0.55, 0.50]], F32)
    x_old = np.array([[0.58, 0.44, 0.50, 0.52]], F32)
    x_best = np.array([[0.70, 0.30, 0.45, 0.65]], F32)
    grad_best = np.array([[1, -1, 0, 2]], F32)
    grad = -grad_best
    xa, xo, xb, xf, gb = R.step(x_adv, x_old, x_best, x_best.copy(), grad_best, x0, grad, [R.RESTART], [st], eps, a)
    assert np.array_equal(xo, x_best) and np.array_equal(xb, x_best) and np.array_equal(gb, grad_best)
    g2 = x_best - x_old                                   # the momentum term sees the OLD x_old
    z = np.clip(x_best + st * np.sign(grad_best), 0.25, 0.75).astype(F32)
    want = np.clip((x_best + (z - x_best) * a) + g2 * (F32(1) - a), 0.25, 0.75).astype(F32)
    assert np.array_equal(xa, want)
    # improved and restart together: x_best becomes x_adv first, so the point does not move before the update
    xa2, xo2, xb2, _, gb2 = R.step(x_adv, x_old, x_best, x_best.copy(), grad_best, x0, grad, [R.RESTART | R.IMPROVED], [st], eps, a)
    assert np.array_equal(xo2, x_adv) and np.array_equal(xb2, x_adv) and np.array_equal(gb2, grad)
    # last: copies only
    xa3, xo3, _, xf3, _ = R.step(x_adv, x_old, x_best, x_best.copy(), grad_best, x0, grad, [R.FOOLED | R.RESTART], [st], eps, a, last=True)
    assert np.array_equal(xa3, x_adv) and np.array_equal(xo3, x_old) and np.array_equal(xf3, x_adv)


def test_one_step_from_x_is_the_fgsm_point_for_every_improved_image():
    cfg, w, lora, x, _ = make_case(batch=8, seed=5)
    y = O.vit_forward(w, cfg, O.normalise(x), lora).argmax(1)
    eps = 0.5 / 255
    res = R.attack(w, cfg, x, y, eps, 1, lora)
    _, g, _, _ = R.eval_point(w, cfg, x, y, lora)
    fgsm = torch.clamp(x + F32(eps) * torch.sign(torch.from_numpy(g)), 0, 1).numpy()
    improved = res["trace_loss"][1] > res["trace_loss"][0]
    assert improved.any()
    for b in np.nonzero(improved)[0]:
        assert np.array_equal(res["x_best"][b], fgsm[b]), b
    for b in np.nonzero(~improved)[0]:
        assert np.array_equal(res["x_best"][b], x[b].numpy()), b
    assert (res["trace_step"][0] == F32(2) * F32(eps)).all()
