"""Reference restatement of Auto-PGD (APGD-CE, L-inf; Croce & Hein 2020) for the tests of vl_apgd_attack.

This is the algorithm text of DESIGN.md section 3.9 written a second time, in numpy float32 -- NOT the autoattack package
(`autoattack` / `torchattacks` are not installed; the text is a restatement of autopgd_base.py from memory, so parity with
the package is unpinned).  Three pieces:

    schedule(n_iter)        the checkpoints (i, k)
    StateMachine            steps 2-4: best loss, robust flag, checkpoint test, step size; one flag word per image and iteration
    step(...)               step 1 and the copies, as vl_apgd_step applies them (float32, every operation rounded on its own)
    attack(...)             the whole attack over the CPU oracle's forward (O.vit_forward) and torch autograd

Per image; L-inf, loss = CE, eot_iter = 1.  P(v) = clamp(min(max(v, x - eps), x + eps), 0, 1).
"""
import numpy as np
import torch

from helpers import O

F32 = np.float32
IMPROVED, FOOLED, RESTART = 1, 2, 4


def schedule(n_iter):
    k, k_min, dec = max(int(.22 * n_iter), 1), max(int(.06 * n_iter), 1), max(int(.03 * n_iter), 1)
    out, cnt = [], 0
    for i in range(n_iter):
        cnt += 1
        if cnt == k:
            out.append((i, k))
            k, cnt = max(k - dec, k_min), 0
    return out


class StateMachine:
    """Vectorised over the batch.  start(loss, pred) is the evaluation of the start point, observe(i, loss, pred) that of the
    point iteration i made; both return the flag words [B].  `step` is then the step size the NEXT update uses."""

    def __init__(self, batch, n_iter, eps, rho=.75):
        self.B, self.N, self.eps, self.rho = batch, n_iter, F32(eps), F32(rho)
        self.k = max(int(.22 * n_iter), 1)
        self.k_min = max(int(.06 * n_iter), 1)
        self.dec = max(int(.03 * n_iter), 1)
        self.cnt = 0
        self.loss_steps = np.zeros((n_iter, batch), F32)

    def start(self, loss, pred):
        loss, pred = np.asarray(loss, F32), np.asarray(pred, bool)
        self.loss_best = loss.copy()
        self.loss_best_last = loss.copy()
        self.robust = pred.copy()
        self.step = np.full(self.B, F32(2) * self.eps, F32)
        self.reduced_last = np.ones(self.B, bool)
        return np.full(self.B, IMPROVED | FOOLED, np.int32)        # x_best = x_best_adv = x_adv, grad_best = grad

    def observe(self, i, loss, pred):
        loss, pred = np.asarray(loss, F32), np.asarray(pred, bool)
        flags = np.zeros(self.B, np.int32)
        self.robust &= pred
        flags[~pred] |= FOOLED
        self.loss_steps[i] = loss
        imp = loss > self.loss_best
        self.loss_best = np.where(imp, loss, self.loss_best)
        flags[imp] |= IMPROVED
        self.cnt += 1
        if self.cnt == self.k:
            t = np.zeros(self.B, np.int64)
            for c in range(self.k):
                hi = self.loss_steps[i - c]
                lo = self.loss_steps[i - c - 1] if i - c - 1 >= 0 else np.zeros(self.B, F32)     # index -1 reads 0
                t += hi > lo
            osc = t.astype(F32) <= F32(self.k) * self.rho
            noimp = ~self.reduced_last & (self.loss_best_last >= self.loss_best)
            red = osc | noimp
            self.reduced_last = red.copy()
            self.loss_best_last = self.loss_best.copy()
            self.step = np.where(red, self.step / F32(2), self.step).astype(F32)
            flags[red] |= RESTART
            self.k = max(self.k - self.dec, self.k_min)
            self.cnt = 0
        return flags


def replay(loss_trace, pred_trace, eps, rho=.75):
    """Feeds a recorded trace (rows 0 .. N: the start point, then each iteration's point) through the state machine.
    Returns (step [N, B] -- the step size iteration i's update uses --, flags [N + 1, B], loss_best [B], robust [B])."""
    loss_trace, pred_trace = np.asarray(loss_trace, F32), np.asarray(pred_trace, bool)
    n, b = loss_trace.shape[0] - 1, loss_trace.shape[1]
    sm = StateMachine(b, n, eps, rho)
    flags = [sm.start(loss_trace[0], pred_trace[0])]
    steps = [sm.step.copy()]
    for i in range(n):
        flags.append(sm.observe(i, loss_trace[i + 1], pred_trace[i + 1]))
        steps.append(sm.step.copy())
    return np.stack(steps[:n]), np.stack(flags), sm.loss_best.copy(), sm.robust.copy()


def _proj(v, x0, eps):
    return np.clip(np.minimum(np.maximum(v, x0 - eps), x0 + eps), F32(0), F32(1))


def step(x_adv, x_old, x_best, x_best_adv, grad_best, x0, grad, flags, step_size, eps, a, last=False):
    """What vl_apgd_step does to [B, ...] float32 arrays (returns new copies of the five state arrays): the copies the flags
    ask for, then -- unless `last` -- step 1 of the next iteration."""
    x_adv, x_old, x_best, x_best_adv, grad_best = (np.array(t, F32) for t in (x_adv, x_old, x_best, x_best_adv, grad_best))
    x0, grad = np.asarray(x0, F32), np.array(grad, F32)
    eps, a = F32(eps), F32(a)
    for b in range(x_adv.shape[0]):
        f = int(flags[b])
        if f & IMPROVED:
            x_best[b], grad_best[b] = x_adv[b], grad[b]
        if f & FOOLED:
            x_best_adv[b] = x_adv[b]
        if last:
            continue
        if f & RESTART:                                  # after the improved copy; x_old is left alone
            x_adv[b], grad[b] = x_best[b], grad_best[b]
        st = F32(step_size[b])
        g2 = x_adv[b] - x_old[b]
        x_old[b] = x_adv[b]
        z = _proj(x_adv[b] + st * np.sign(grad[b]), x0[b], eps)
        x_adv[b] = _proj((x_adv[b] + (z - x_adv[b]) * a) + g2 * (F32(1) - a), x0[b], eps)
    return x_adv, x_old, x_best, x_best_adv, grad_best


def eval_point(w, cfg, x01, labels, lora=None):
    """(per-image CE [B], dCE/dx (sum over images: only its sign is used), pred [B]) at pixels x01 in [0,1]."""
    x = torch.as_tensor(x01).clone().detach().requires_grad_(True)
    logits = O.vit_forward(w, cfg, O.normalise(x), lora)
    loss = torch.nn.functional.cross_entropy(logits, labels, reduction="none")
    (g,) = torch.autograd.grad(loss.sum(), x)
    return loss.detach().numpy().astype(F32), g.numpy().astype(F32), (logits.argmax(1) == labels).numpy(), logits.detach()


def attack(w, cfg, x01, labels, eps, n_iter, lora=None, x_init=None, rho=.75):
    """The whole attack from x (or x_init) on the CPU oracle.  Returns a dict with x_best, x_best_adv, loss_best, robust and the
    traces (loss [N + 1, B], step [N, B], pred [N + 1, B], margin [N + 1, B] = top-1 minus top-2 logit)."""
    x0 = np.asarray(x01, F32)
    b = x0.shape[0]
    x_adv = np.clip(np.asarray(x_init if x_init is not None else x01, F32), F32(0), F32(1))
    x_old = x_adv.copy()
    x_best, x_best_adv, grad_best = x_adv.copy(), x_adv.copy(), np.zeros_like(x_adv)
    sm = StateMachine(b, n_iter, eps, rho)
    tl, ts, tp, tm = [], [], [], []
    for j in range(n_iter + 1):
        loss, grad, pred, logits = eval_point(w, cfg, torch.from_numpy(x_adv), labels, lora)
        top2 = logits.topk(2, dim=1).values
        tm.append((top2[:, 0] - top2[:, 1]).numpy())
        flags = sm.start(loss, pred) if j == 0 else sm.observe(j - 1, loss, pred)
        tl.append(loss)
        tp.append(pred)
        last = j == n_iter
        if not last:
            ts.append(sm.step.copy())
        x_adv, x_old, x_best, x_best_adv, grad_best = step(x_adv, x_old, x_best, x_best_adv, grad_best, x0, grad, flags, sm.step,
                                                           eps, 1.0 if j == 0 else .75, last)
    return {"x_best": x_best, "x_best_adv": x_best_adv, "loss_best": sm.loss_best.copy(), "robust": sm.robust.copy(),
            "trace_loss": np.stack(tl), "trace_step": np.stack(ts), "trace_pred": np.stack(tp), "trace_margin": np.stack(tm)}
