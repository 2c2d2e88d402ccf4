"""Known answers of tests/square_ref.py, the numpy restatement of the Square attack the GPU tests hold vl_square_attack to
(DESIGN.md section 3.10).  No GPU."""
import numpy as np

import square_ref as R
from helpers import O, make_case

F32 = np.float32


def _changes(s):
    return [(j + 1, s[j]) for j in range(len(s)) if j == 0 or s[j] != s[j - 1]]


def test_mix64_is_the_splitmix64_finaliser():
    assert R.mix64(0) == 0xE220A8397B1DCDAF              # the first output of splitmix64 seeded with 0
    assert R.draw(1, 0, 1, 0) == 0x3860BA74A9D128B4
    assert R.draw(1, 0, 1, 0) != R.draw(1, 1, 1, 0) != R.draw(1, 0, 2, 0)
    assert R.draw(2 ** 64 + 1, 0, 1, 0) == R.draw(1, 0, 1, 0)        # the key is taken mod 2^64


def test_sides_224_5000():
    s = R.sides(224, 0.8, 5000)
    assert s[0] == 200 == round((0.8 * 224 * 224) ** 0.5) and s[-1] == 9 == round((0.8 / 512 * 224 * 224) ** 0.5)
    # it = int((j - 1) / 5000 * 10000) = 2 (j - 1) exceeds 10 first at j = 7, 50 at j = 27, ..., 8000 at j = 4002
    assert _changes(s) == [(1, 200), (7, 142), (27, 100), (102, 71), (252, 50), (502, 35), (1002, 25), (2002, 18), (3002, 13),
                           (4002, 9)]
    assert all(a >= b for a, b in zip(s, s[1:]))


def test_sides_64_50_and_10():
    assert _changes(R.sides(64, 0.8, 50)) == [(1, 57), (2, 29), (3, 20), (4, 14), (7, 10), (12, 7), (22, 5), (32, 4), (42, 3)]
    assert R.sides(64, 0.8, 10) == [57, 14, 10, 7, 7, 5, 5, 4, 4, 3]       # a short schedule jumps over halvings
    assert R.sides(64, 1.0, 1) == [64]                                     # p = 1: the whole image
    assert R.sides(8, 0.001, 3) == [1, 1, 1]                               # never below one pixel


def test_p_selection_thresholds_are_strict():
    n = 10000                                   # it = j - 1
    assert R.p_selection(1.0, 11, n) == 1.0 and R.p_selection(1.0, 12, n) == 0.5
    assert R.p_selection(1.0, 8001, n) == 1 / 256 and R.p_selection(1.0, 8002, n) == 1 / 512
    assert R.p_selection(0.8, 1, n) == float(F32(0.8))       # p_init is the float32 the ABI carries


def test_draws_stay_inside_the_image():
    S = 64
    for s in (1, 2, 5, 13, 63, 64):
        hs, ws, sg = set(), set(), set()
        for g in range(4):
            for j in range(1, 200):
                h, w, s2, signs = R.proposal(3, g, j, S, s)
                assert s2 == s and 0 <= h <= S - s and 0 <= w <= S - s and 0 <= signs < 8
                hs.add(h), ws.add(w), sg.add(signs)
        if s == S:
            assert hs == ws == {0}
        else:
            assert min(hs) == 0 == min(ws) and max(hs) == S - s == max(ws)
        assert sg == set(range(8))


def test_stripes_are_constant_along_columns():
    g = np.random.default_rng(0)
    x0 = g.random((2, 3, 8, 8)).astype(F32)
    x0[0, 0, 0, :4] = [0, 1, 0, 1]
    eps = 8 / 255
    a = R.stripes(x0, eps, seed=1)
    d = a - x0
    assert np.abs(d).max() <= F32(eps) + 1e-7 and a.min() >= 0 and a.max() <= 1
    inner = (x0 > 0.1) & (x0 < 0.9)
    sign = np.sign(np.where(inner, d, 0))
    for b in range(2):
        for c in range(3):
            for col in range(8):
                v = sign[b, c, :, col]
                assert len(set(v[v != 0])) <= 1
    assert not np.array_equal(R.stripes(x0, eps, seed=1)[0], R.stripes(x0, eps, seed=1, image_offset=1)[0])
    assert np.array_equal(R.stripes(x0, eps, seed=1)[1], R.stripes(x0[1:], eps, seed=1, image_offset=1)[0])


def test_step_rule():
    S = 8
    x0 = np.full((1, 3, S, S), 0.5, F32)
    x0[0, 0, 0, 0], x0[0, 0, 0, 1] = 0.0, 1.0
    cur, best = np.full_like(x0, 0.25), np.full_like(x0, 0.75)
    eps = F32(0.125)
    prev, nxt = np.array([[0, 0, 4, 0]]), np.array([[2, 2, 4, 0b101]])
    c, b = R.step(cur, best, x0, [R.PREV | R.ACCEPT | R.NEXT], prev, nxt, eps)
    assert (b[0, :, :4, :4] == 0.25).all() and (b[0, :, 4:, :] == 0.75).all() and (b[0, :, :, 4:] == 0.75).all()
    assert (c[0, 0, 2:6, 2:6] == 0.625).all() and (c[0, 1, 2:6, 2:6] == 0.375).all() and (c[0, 2, 2:6, 2:6] == 0.625).all()
    assert (c[0, :, :2, :] == 0.25).all() and (c[0, :, 6:, :] == 0.25).all()
    c, b = R.step(cur, best, x0, [R.PREV | R.NEXT], prev, nxt, eps)          # rejected: x_cur comes back, x_best is not written
    assert np.array_equal(b, best)
    assert (c[0, :, :2, :4] == 0.75).all() and (c[0, :, :4, :2] == 0.75).all() and (c[0, 1, 2:6, 2:6] == 0.375).all()
    assert (c[0, :, 6:, :] == 0.25).all()
    c, b = R.step(cur, best, x0, [0], prev, nxt, eps)                         # neither window
    assert np.array_equal(c, cur) and np.array_equal(b, best)
    c, _ = R.step(cur, best, x0, [R.NEXT], prev, np.array([[0, 0, 2, 0b001]]), eps)     # the clamp at 0 and 1
    assert c[0, 0, 0, 0] == 0.125 and c[0, 0, 0, 1] == 1.0 and c[0, 1, 0, 0] == 0.375


def test_state_machine_on_hand_made_rows():
    n, S = 5, 64
    nan = np.nan
    #            decreasing  constant  ties      frozen@0  crosses mid  NaN start  NaN later
    rows = [[1.0, 1.0, 1.0, -0.5, 1.0, nan, 1.0],
            [0.9, 1.0, 1.0, -0.5, 0.5, 2.0, nan],
            [0.8, 1.0, 0.5, -0.5, -0.1, 3.0, 0.5],
            [0.7, 1.0, 0.5, -0.5, -0.1, 1.0, 0.6],
            [0.6, 1.0, 0.4, -0.5, -0.1, 1.0, 0.4],
            [-0.1, 1.0, 0.4, -0.5, -0.1, 0.5, 0.4]]
    flags, tw, mm, q, rob = R.replay(np.array(rows, F32), S, seed=2)
    A, P, N = R.ACCEPT, R.PREV, R.NEXT
    assert flags[:, 0].tolist() == [N, P | A | N, P | A | N, P | A | N, P | A | N, P | A]
    assert flags[:, 1].tolist() == [N, P | N, P | N, P | N, P | N, P]                   # an equal margin is not accepted
    assert flags[:, 2].tolist() == [N, P | N, P | A | N, P | N, P | A | N, P]
    assert flags[:, 3].tolist() == [0] * 6                                              # frozen at the start: no proposal ever
    assert flags[:, 4].tolist() == [N, P | A | N, P | A, 0, 0, 0]                       # frozen once the margin is <= 0
    assert flags[:, 5].tolist() == [N, P | A | N, P | N, P | A | N, P | N, P | A]       # NaN at the start: margin_min = +inf
    assert flags[:, 6].tolist() == [N, P | N, P | A | N, P | N, P | A | N, P]           # NaN is never accepted
    assert mm.tolist() == [F32(-0.1), 1.0, F32(0.4), -0.5, F32(-0.1), 0.5, F32(0.4)]
    assert q.tolist() == [6, 6, 6, 1, 3, 6, 6]
    assert rob.tolist() == [False, True, True, False, False, True, True]
    sides = R.sides(S, 0.8, n)
    for b in range(7):
        for j in range(1, n + 1):
            active = bool(flags[j - 1, b] & N)
            want = list(R.proposal(2, b, j, S, sides[j - 1])) if active else [0, 0, 0, 0]
            if active:
                want[3] |= 8 | (16 if flags[j, b] & A else 0)
            assert tw[j - 1, b].tolist() == want, (b, j)


def test_image_offset_cuts_the_batch_anywhere():
    rows = np.linspace(1, 0.5, 11, dtype=F32)[:, None].repeat(8, 1)
    whole = R.replay(rows, 64, seed=4)[1]
    lo, hi = R.replay(rows[:, :4], 64, seed=4)[1], R.replay(rows[:, 4:], 64, seed=4, image_offset=4)[1]
    assert np.array_equal(whole, np.concatenate([lo, hi], 1))
    assert not np.array_equal(lo, hi)


def test_cpu_attack_known_answer():
    """eps = 8/255, N = 50, seed = 1 on make_case(batch=8, seed=5) with the oracle's clean argmax as labels: images 1 and 4 are
    fooled at margins -0.089 / -0.069, far from any rounding; the robust images end at 0.15 / 0.045 / 0.30 / 0.18."""
    cfg, w, lora, x, _ = make_case(batch=8, seed=5)
    y = O.vit_forward(w, cfg, O.normalise(x), lora).argmax(1)
    r = R.attack(w, cfg, x.numpy(), y.numpy(), 8 / 255, 50, lora, seed=1)
    assert r["robust"].astype(int).tolist() == [1, 0, 1, 1, 0, 0, 0, 1]
    assert np.allclose(r["margin_min"][[0, 1, 3, 4, 7]], [0.1538, -0.0894, 0.2993, -0.0689, 0.1827], atol=2e-3)
    assert r["queries"][r["robust"]].tolist() == [51] * 4 and r["queries"][1] == 1
    assert np.abs(r["x_best"] - x.numpy()).max() <= F32(8 / 255) + 1e-6
    # the result is the state machine on its own trace, and x_best is the accepted windows applied to the stripes
    flags, tw, mm, q, rob = R.replay(r["trace_margin"], 64, seed=1)
    assert np.array_equal(tw, r["trace_win"]) and np.array_equal(mm, r["margin_min"]) and np.array_equal(q, r["queries"])
    frozen = ~r["robust"]
    assert np.array_equal(r["trace_margin"][-1][frozen], r["margin_min"][frozen])
