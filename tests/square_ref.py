"""Reference restatement of the Square attack (Andriushchenko et al. 2020; L-inf, margin loss, rescaled schedule) for the tests of
vl_square_attack.

This is the algorithm text of DESIGN.md section 3.10 written a second time, in numpy float32 and Python integers -- NOT the
autoattack package (`autoattack` / `torchattacks` are not installed; the text is a restatement of square.py and the paper from
memory, so parity with the package is unpinned).  Two deliberate deviations from the package: the window and its signs are drawn
per image (global index g = image_offset + b), and the window is written as clamp(x0 +- eps, 0, 1) directly.

    mix64, draw             the counter-based generator r(g, j, k) = mix64(key ^ (g << 32) ^ (j << 2) ^ k)
    p_selection, side       the schedule: p of proposal j, and the window side it gives
    proposal                (h, w, s, signs) of proposal j for image g
    stripes                 the start point
    step                    the per-pixel rule of one replay, as vl_square_step applies it
    StateMachine, replay    accept / reject, margin_min, queries, the flag words and windows over a margin trace
    attack                  the whole attack over the CPU oracle's forward (O.vit_forward)
"""
import math

import numpy as np
import torch

from helpers import O

F32 = np.float32
M64 = (1 << 64) - 1
PREV, ACCEPT, NEXT = 1, 2, 4
THRESHOLDS = (10, 50, 200, 500, 1000, 2000, 4000, 6000, 8000)


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, g, j, k):
    key = (int(seed) * 0xD1342543DE82EF95) & M64
    return mix64(key ^ ((int(g) << 32) & M64) ^ (int(j) << 2) ^ int(k))


def p_selection(p_init, j, n_queries):
    """p of proposal j = 1 .. N.  p_init is the float32 the C ABI carries, the arithmetic is double."""
    it = int((j - 1) / n_queries * 10000)
    k = sum(1 for t in THRESHOLDS if it > t)
    return float(F32(p_init)) / 2 ** k


def side(S, p_init, j, n_queries):
    return min(S, max(1, round(math.sqrt(p_selection(p_init, j, n_queries) * S * S))))      # round(): half to even


def sides(S, p_init, n_queries):
    return [side(S, p_init, j, n_queries) for j in range(1, n_queries + 1)]


def proposal(seed, g, j, S, s):
    """(h, w, s, signs): the window of proposal j for the image with global index g; bit c of signs: channel c is +eps."""
    h = ((draw(seed, g, j, 0) >> 32) * (S - s + 1)) >> 32
    w = ((draw(seed, g, j, 1) >> 32) * (S - s + 1)) >> 32
    return h, w, s, (draw(seed, g, j, 2) >> 40) & 7


def stripes(x0, eps, seed, image_offset=0):
    x0 = np.asarray(x0, F32)
    B, C, S, _ = x0.shape
    sign = np.empty((B, C, 1, S), F32)
    for b in range(B):
        for c in range(C):
            for col in range(S):
                sign[b, c, 0, col] = 1 if (draw(seed, image_offset + b, c * S + col, 3) >> 40) & 1 else -1
    return np.clip(x0 + F32(eps) * sign, F32(0), F32(1)).astype(F32)


def step(x_cur, x_best, x0, flags, win_prev, win_next, eps):
    """What vl_square_step does to [B, 3, S, S] float32 arrays (returns new copies of x_cur and x_best).  Per pixel, in order:
    in the previous window: accepted -> x_best = x_cur, else x_cur = x_best; in the next window: x_cur = clamp(x0 +- eps, 0, 1)."""
    x_cur, x_best = np.array(x_cur, F32), np.array(x_best, F32)
    x0, eps = np.asarray(x0, F32), F32(eps)
    for b in range(x_cur.shape[0]):
        f = int(flags[b])
        if f & PREV:
            h, w, s, _ = (int(v) for v in win_prev[b])
            if f & ACCEPT:
                x_best[b, :, h:h + s, w:w + s] = x_cur[b, :, h:h + s, w:w + s]
            else:
                x_cur[b, :, h:h + s, w:w + s] = x_best[b, :, h:h + s, w:w + s]
        if f & NEXT:
            h, w, s, sg = (int(v) for v in win_next[b])
            for c in range(x_cur.shape[1]):
                sig = eps if (sg >> c) & 1 else -eps
                x_cur[b, c, h:h + s, w:w + s] = np.clip(x0[b, c, h:h + s, w:w + s] + sig, F32(0), F32(1))
    return x_cur, x_best


class StateMachine:
    """Per image b (global index image_offset + b).  observe(j, margin) is replay j; it returns the flag words [B] and leaves
    win_prev / win_next [B, 4], margin_min, queries and trace_win as the track kernel does.  A margin that is not finite is never
    accepted; at replay 0 it leaves margin_min = +inf (the image stays active)."""

    def __init__(self, batch, n_queries, S, p_init=0.8, seed=0, image_offset=0):
        self.B, self.N, self.S, self.seed, self.off = batch, n_queries, S, seed, image_offset
        self.side = [0] + sides(S, p_init, n_queries)
        self.margin_min = np.zeros(batch, F32)
        self.queries = np.zeros(batch, np.int32)
        self.flags = np.zeros(batch, np.int32)
        self.win_prev = np.zeros((batch, 4), np.int32)
        self.win_next = np.zeros((batch, 4), np.int32)
        self.trace_win = np.zeros((n_queries, batch, 4), np.int32)

    def observe(self, j, margin):
        margin = np.asarray(margin, F32)
        new = np.zeros(self.B, np.int32)
        for b in range(self.B):
            m = margin[b]
            finite = bool(np.isfinite(m))
            if j == 0:
                self.margin_min[b] = m if finite else F32(np.inf)
                self.queries[b] = 1
            elif self.flags[b] & NEXT:
                self.queries[b] += 1
                new[b] |= PREV
                self.win_prev[b] = self.win_next[b]
                if finite and m < self.margin_min[b]:
                    self.margin_min[b] = m
                    new[b] |= ACCEPT
                    self.trace_win[j - 1, b, 3] |= 16
            if j < self.N and self.margin_min[b] > 0:
                h, w, s, sg = proposal(self.seed, self.off + b, j + 1, self.S, self.side[j + 1])
                self.win_next[b] = (h, w, s, sg)
                self.trace_win[j, b] = (h, w, s, sg | 8)
                new[b] |= NEXT
        self.flags = new
        return new.copy()

    @property
    def robust(self):
        return self.margin_min > 0


def replay(trace_margin, S, p_init=0.8, seed=0, image_offset=0):
    """Feeds a recorded margin trace [N + 1, B] through the state machine.  Returns (flags [N + 1, B], trace_win [N, B, 4],
    margin_min [B], queries [B], robust [B])."""
    trace_margin = np.asarray(trace_margin, F32)
    n, b = trace_margin.shape[0] - 1, trace_margin.shape[1]
    sm = StateMachine(b, n, S, p_init, seed, image_offset)
    flags = [sm.observe(j, trace_margin[j]) for j in range(n + 1)]
    return np.stack(flags), sm.trace_win.copy(), sm.margin_min.copy(), sm.queries.copy(), sm.robust.copy()


def margin(logits, labels):
    """z_y - max_{j != y} z_j, float32."""
    z = np.array(logits, F32)
    idx = np.arange(z.shape[0])
    zy = z[idx, labels].copy()
    z[idx, labels] = -np.inf
    return (zy - z.max(1)).astype(F32)


def attack(w, cfg, x01, labels, eps, n_queries, lora=None, p_init=0.8, seed=0, image_offset=0):
    """The whole attack on the CPU oracle.  Returns a dict with x_best, margin_min, queries, robust, trace_margin [N + 1, B] and
    trace_win [N, B, 4]."""
    x0 = np.asarray(x01, F32)
    labels = np.asarray(labels)
    B, _, S, _ = x0.shape
    x_cur = stripes(x0, eps, seed, image_offset)
    x_best = x_cur.copy()
    sm = StateMachine(B, n_queries, S, p_init, seed, image_offset)
    tm = []
    for j in range(n_queries + 1):
        with torch.no_grad():
            logits = O.vit_forward(w, cfg, O.normalise(torch.from_numpy(x_cur)), lora).numpy()
        m = margin(logits, labels)
        tm.append(m)
        flags = sm.observe(j, m)
        x_cur, x_best = step(x_cur, x_best, x0, flags, sm.win_prev, sm.win_next, eps)
    return {"x_best": x_best, "margin_min": sm.margin_min.copy(), "queries": sm.queries.copy(), "robust": sm.robust.copy(),
            "trace_margin": np.stack(tm), "trace_win": sm.trace_win.copy()}
