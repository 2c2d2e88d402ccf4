"""Reference restatement of APGD-T (targeted Auto-PGD on the DLR loss, L-inf) for the tests of vl_apgdt_attack.

This is the algorithm text of DESIGN.md section 3.11 written a second time -- NOT the autoattack package (`autoattack` /
`torchattacks` are not installed; the text is a restatement of autopgd_base.py's APGDAttack_targeted from memory, so parity with
the package is unpinned).  The iteration is apgd_ref's (StateMachine, step); what is new:

    dlr_targeted(logits, y, t, dtype)   the loss and D * dloss/dlogits per row, in float64 or in float32 with the kernel's order
    targets(logits, y, n)               the n most likely classes other than the label, ties by the lower index
    attack(...)                         every target and restart over the CPU oracle and torch autograd, and the fold over runs

pi = the descending order of a row (value descending, index ascending); N = z_y - z_t; D = (z_pi1 - (z_pi3 + z_pi4) / 2) + 1e-12;
loss = -N / D (maximised).
"""
import numpy as np
import torch

import apgd_ref as A
from helpers import O

F32 = np.float32
# The whole-attack case of the tests -- make_case(batch=8, seed=5), image 0 clean-wrong -- chosen on the CPU so that the reference
# fools some images and leaves some robust (tests/test_apgdt_ref_cpu.py records the counts); the GPU tests use the same numbers.
CASE_EPS, CASE_STEPS, CASE_N_TARGET = 0.5 / 255, 10, 3


def order(z):
    """Indices of one row by value descending, index ascending."""
    z = np.asarray(z)
    return np.lexsort((np.arange(z.shape[0]), -z))


def dlr_targeted(logits, y, t, dtype=np.float64):
    """(loss [B], D * dloss/dlogits [B, C]) in `dtype`; with float32 every operation is rounded on its own in the order
    dlr_targeted_loss_kernel uses: n = z_y - z_t; h = (z_pi3 + z_pi4) * .5; d = (z_pi1 - h) + 1e-12; q = n / d; loss = -q;
    row = -(a - q * w), a = [c == y] - [c == t], w = ([c == pi1] - .5 [c == pi3]) - .5 [c == pi4]."""
    z = np.asarray(logits, dtype)
    B, C = z.shape
    loss = np.zeros(B, dtype)
    grad = np.zeros((B, C), dtype)
    half, tiny = dtype(0.5), dtype(1e-12)
    for b in range(B):
        pi = order(z[b])
        yb, tb = int(y[b]), int(t[b])
        n = z[b, yb] - z[b, tb]
        h = (z[b, pi[2]] + z[b, pi[3]]) * half
        d = (z[b, pi[0]] - h) + tiny
        q = dtype(n / d)
        a = np.zeros(C, dtype)
        a[yb] += dtype(1)
        a[tb] -= dtype(1)
        w = np.zeros(C, dtype)
        w[pi[0]] = dtype(1)
        w[pi[2]] = dtype(-0.5)
        w[pi[3]] = dtype(-0.5)
        loss[b] = -q
        grad[b] = -(a - q * w)
    return loss, grad


def targets(logits, y, n):
    """[n, B] int32: row k = the class with the (k + 1)-th largest logit among the classes != y[b], the lower index first among
    equal logits."""
    z = np.asarray(logits)
    out = np.zeros((n, z.shape[0]), np.int32)
    for b in range(z.shape[0]):
        pi = [c for c in order(z[b]) if c != int(y[b])]
        out[:, b] = pi[:n]
    return out


def dlr_torch(logits, y, t):
    """The loss per image as a torch expression (autograd gives dloss/dlogits itself, without the factor D)."""
    srt = torch.sort(logits, dim=1, descending=True, stable=True).values
    zy = logits.gather(1, y.view(-1, 1)).squeeze(1)
    zt = logits.gather(1, t.view(-1, 1)).squeeze(1)
    return -(zy - zt) / (srt[:, 0] - 0.5 * (srt[:, 2] + srt[:, 3]) + 1e-12)


def eval_point(w, cfg, x01, labels, tgt, lora=None):
    """(per-image DLR loss [B], dloss/dx summed over images (only its sign is used), pred [B], logits) at pixels x01 in [0,1]."""
    x = torch.as_tensor(x01).clone().detach().requires_grad_(True)
    logits = O.vit_forward(w, cfg, O.normalise(x), lora)
    loss = dlr_torch(logits, labels, tgt)
    (g,) = torch.autograd.grad(loss.sum(), x)
    return loss.detach().numpy().astype(F32), g.numpy().astype(F32), (logits.argmax(1) == labels).numpy(), logits.detach()


def random_start(x0, eps, seed):
    """x0 + eps t / max|t| per image, t ~ U(-1, 1), clamped to [0, 1] (the library draws from its own counter-based generator:
    the points differ, the rule is the same)."""
    rng = np.random.default_rng(seed)
    t = (rng.random(x0.shape) * 2 - 1).astype(F32)
    mx = np.abs(t).reshape(t.shape[0], -1).max(1).reshape(-1, 1, 1, 1)
    return np.clip(x0 + (F32(eps) * t) / mx, F32(0), F32(1)).astype(F32)


def one_run(w, cfg, x0, labels, tgt, eps, n_iter, seed, lora=None, rho=.75):
    """One APGD run on the DLR loss towards tgt from a random start: (x_best_adv, loss_best [B], robust [B])."""
    b = x0.shape[0]
    x_adv = random_start(x0, eps, seed)
    x_old = x_adv.copy()
    x_best, x_best_adv, grad_best = x_adv.copy(), x_adv.copy(), np.zeros_like(x_adv)
    sm = A.StateMachine(b, n_iter, eps, rho)
    for j in range(n_iter + 1):
        loss, grad, pred, _ = eval_point(w, cfg, torch.from_numpy(x_adv), labels, tgt, lora)
        flags = sm.start(loss, pred) if j == 0 else sm.observe(j - 1, loss, pred)
        x_adv, x_old, x_best, x_best_adv, grad_best = A.step(x_adv, x_old, x_best, x_best_adv, grad_best, x0, grad, flags, sm.step,
                                                             eps, 1.0 if j == 0 else .75, j == n_iter)
    return x_best_adv, sm.loss_best.copy(), sm.robust.copy()


def fold(x_adv, still, fooled_by, run, x_best_adv, run_robust):
    """The fold after one run (in place on the three arrays): a still-robust image that the run fooled takes the run's point."""
    take = still & ~run_robust
    x_adv[take] = x_best_adv[take]
    fooled_by[take] = run
    still &= run_robust


def attack(w, cfg, x01, labels, eps, n_iter, n_target, n_restarts, lora=None, rho=.75, seed=0, targets_in=None):
    """The whole attack on the CPU oracle.  Returns a dict with x_adv, robust, clean_correct, targets [n_target, B], fooled_by,
    loss_best [runs, B] and robust_run [runs, B]; run = k * n_restarts + r uses the seed `seed + run`."""
    x0 = np.asarray(x01, F32)
    logits = O.vit_forward(w, cfg, O.normalise(torch.from_numpy(x0)), lora).detach()
    clean = (logits.argmax(1) == labels).numpy()
    tg = targets(logits.numpy(), labels.numpy(), n_target) if targets_in is None else np.asarray(targets_in, np.int32)
    x_adv, still = x0.copy(), clean.copy()
    fooled_by = np.full(x0.shape[0], -1, np.int32)
    lb, rr = [], []
    for k in range(n_target):
        for r in range(n_restarts):
            run = k * n_restarts + r
            xb, loss_best, robust = one_run(w, cfg, x0, labels, torch.from_numpy(tg[k].astype(np.int64)), eps, n_iter, seed + run,
                                            lora, rho)
            lb.append(loss_best)
            rr.append(robust)
            fold(x_adv, still, fooled_by, run, xb, robust)
    return {"x_adv": x_adv, "robust": still, "clean_correct": clean, "targets": tg, "fooled_by": fooled_by,
            "loss_best": np.stack(lb), "robust_run": np.stack(rr)}
