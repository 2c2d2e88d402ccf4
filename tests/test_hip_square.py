"""GPU tests of the Square attack (L-inf, margin loss): vl_square_step, vl_debug_square_track, vl_square_attack and the Square /
AutoAttack facade.

The reference is tests/square_ref.py, a numpy float32 / Python-integer restatement of the algorithm text (DESIGN.md section
3.10; a restatement of the autoattack package from memory -- parity with the package is unpinned).  The kernels are held to it
bit for bit on caller-made inputs; the whole attack is held to it through its OWN trace: the bookkeeping must be what the state
machine makes of the margins the GPU saw, the windows must be the reference's draws, and x_best must be, bit for bit, the
accepted windows applied to the stripes.  Full-trajectory parity with the CPU oracle is not asked (an accept decision can sit on a
rounding difference of the forward).  The shared case is that of tests/test_hip_apgd.py: make_case(batch=8, seed=5), labels = the
CPU oracle's clean argmax, 64 x 64 images.  Tolerances of the re-forwarded margin: f16 4e-3, f32 1e-4, bf16 1.5e-2, as there."""
import importlib
import os

import numpy as np
import pytest
import torch

import square_ref as R
from helpers import O, make_case, make_engine, pkg

pytestmark = pytest.mark.gpu

F32 = np.float32
PRECS = ["f16", "bf16", "f32"]
TOL_ACT = {"f16": 4e-3, "f32": 1e-4, "bf16": 1.5e-2}
EPS = 8 / 255
SEED = 1
P, A, N_ = R.PREV, R.ACCEPT, R.NEXT

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


def _cpu(r):
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in r.items()}


def run(prec, n, **kw):
    """One traced attack on the shared case (computed once per key, never modified)."""
    key = (prec, n, tuple(sorted(kw.items())))
    if key not in _RUN:
        c = case()
        r = engine(prec).square_attack(c["x"].cuda(), c["y"].cuda(), EPS, n, seed=SEED, trace=True, **kw)
        torch.cuda.synchronize()
        _RUN[key] = _cpu(r)
    return _RUN[key]


def margins(eng, x, y):
    """The library's forward at the batch size of x and the float32 margin of its logits."""
    logits = eng.forward(x.cuda(), normalise=True).clone()
    torch.cuda.synchronize()
    return R.margin(logits.cpu().numpy(), y.numpy()), logits.cpu()


def same(a, b, what):
    for k, v in a.items():
        if torch.is_tensor(v):
            assert torch.equal(v, b[k].cpu() if torch.is_tensor(b[k]) else b[k]), (what, k)
        else:
            assert v == b[k], (what, k)


# ---- 1. the step kernel, bit for bit ---------------------------------------------------------------------------------------------
def _window_pairs(S):
    q, e = S // 4, S - 13
    return [
        ((0, 0, q), (S // 2, S // 2, q)),                  # disjoint
        ((2, 3, 6), (5, 5, 6)),                            # overlapping
        ((3, 5, 7), (3, 5, 7)),                            # identical
        ((1, 1, 10), (3, 4, 4)),                           # the next one nested in the previous
        ((3, 4, 4), (1, 1, 10)),                           # the previous one nested in the next
        ((0, 0, 1), (S - 1, S - 1, 1)),                    # s = 1 in two corners
        ((S - 1, 0, 1), (S - 1, 0, 1)),                    # s = 1, identical
        ((0, 0, S), (0, 0, S)),                            # s = S twice
        ((0, 0, S), (S - 5, 3, 5)),                        # s = S, then s = 5 at the odd column 3 on the bottom edge
        ((1, 3, 5), (0, 0, S)),                            # odd start column and odd width, then the whole image
        ((0, e, 13), (e, 0, 13)),                          # s = 13 at w = S - 13: top-right corner; bottom-left corner
        ((e, e, 13), (0, 0, 13)),                          # bottom-right and top-left corners
        ((7, S - 9, 9), (7, S - 12, 9)),                   # odd widths on the right edge, overlapping in columns only
    ]


@pytest.mark.parametrize("side", [16, 64])
def test_square_step_kernel_bit_exact(side):
    """Every window pair under every flag word (accept / reject with and without a next proposal, a next proposal alone, neither),
    8 images per launch; x0 holds exact 0 and 1; x_cur and x_best carry unrelated random values, so a pixel written outside the
    union of the two windows, or a copy in the wrong direction, shows.  3 x 64 x 64 windows take several blocks per image."""
    S = side
    g = torch.Generator().manual_seed(side)
    combos = [(p, n, f) for p, n in _window_pairs(S) for f in (P | A | N_, P | N_, P | A, P, N_, 0)]
    combos += [combos[i] for i in range((-len(combos)) % 8)]
    eng = engine("f16")
    for lo in range(0, len(combos), 8):
        grp = combos[lo:lo + 8]
        x0 = torch.rand(8, 3, S, S, generator=g)
        x0.view(-1)[::5] = 0.0
        x0.view(-1)[1::7] = 1.0
        x_cur, x_best = torch.rand(8, 3, S, S, generator=g), torch.rand(8, 3, S, S, generator=g)       # sentinels
        signs = torch.randint(0, 8, (8,), generator=g)
        wp = torch.tensor([[*p, int(torch.randint(0, 8, (1,), generator=g))] for p, _, _ in grp], dtype=torch.int32)
        wn = torch.tensor([[*n, int(signs[i])] for i, (_, n, _) in enumerate(grp)], dtype=torch.int32)
        fl = torch.tensor([f for _, _, f in grp], dtype=torch.int32)
        want_cur, want_best = R.step(x_cur.numpy(), x_best.numpy(), x0.numpy(), fl.numpy(), wp.numpy(), wn.numpy(), EPS)
        dev = [t.cuda().contiguous() for t in (x_cur, x_best, x0, fl, wp, wn)]
        eng.square_step(*dev, EPS)
        torch.cuda.synchronize()
        for name, got, ref in (("x_cur", dev[0], want_cur), ("x_best", dev[1], want_best)):
            bad = (got.cpu().numpy() != ref).reshape(8, -1).sum(1)
            assert not bad.any(), (name, lo, bad.tolist(), grp)
        assert torch.equal(dev[2].cpu(), x0)                                  # the inputs are not written
        # outside the union nothing moved (the reference leaves it alone; said once more in its own terms)
        mask = torch.zeros(8, 1, S, S, dtype=torch.bool)
        for i, ((ph, pw, ps), (nh, nw, ns), f) in enumerate(grp):
            if f & P:
                mask[i, :, ph:ph + ps, pw:pw + ps] = True
            if f & N_:
                mask[i, :, nh:nh + ns, nw:nw + ns] = True
        keep = ~mask.expand(8, 3, S, S)
        assert torch.equal(dev[0].cpu()[keep], x_cur[keep]) and torch.equal(dev[1].cpu()[keep], x_best[keep])


def test_square_step_ignores_a_window_that_leaves_the_image_and_refuses_bad_arguments():
    eng = engine("f16")
    S = 16
    x = [torch.rand(2, 3, S, S).cuda() for _ in range(3)]
    before = [t.clone() for t in x]
    fl = torch.tensor([P | A | N_, P | N_], dtype=torch.int32).cuda()
    wp = torch.tensor([[10, 10, 7, 0], [-1, 0, 4, 0]], dtype=torch.int32).cuda()
    wn = torch.tensor([[0, 12, 5, 7], [0, 0, 17, 7]], dtype=torch.int32).cuda()
    eng.square_step(x[0], x[1], x[2], fl, wp, wn, EPS)
    torch.cuda.synchronize()
    for a, b in zip(x, before):
        assert torch.equal(a, b)
    with pytest.raises(pkg().VitLoraError):
        eng.square_step(x[0], x[1], x[2], fl, wp, wn, float("nan"))


# ---- 2. the start point ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_init_kernel_writes_the_reference_stripes(prec):
    c, eng = case(), engine(prec)
    x = c["x"].clone()
    x.view(-1)[::9] = 0.0
    x.view(-1)[1::11] = 1.0
    for off in (0, 5):
        r = eng.square_attack(x.cuda(), c["y"].cuda(), EPS, 10, seed=3, image_offset=off, count=1)      # replay 0 alone
        got = r["x_best"].cpu().numpy()
        assert r["replays"] == 1 and np.array_equal(got, R.stripes(x.numpy(), EPS, 3, off))
        d = got - x.numpy()
        inner = (x.numpy() > 0.1) & (x.numpy() < 0.9)                   # away from the clamp the offset is +-eps, one sign per column
        sgn = np.where(inner, np.sign(d), np.nan)
        assert np.array_equal(np.nanmax(sgn, axis=2), np.nanmin(sgn, axis=2), equal_nan=True)
        assert np.abs(d).max() <= F32(EPS) + 1e-7
        assert (r["queries"].cpu() == 1).all()


# ---- 3. the track kernel, exactly ------------------------------------------------------------------------------------------------
def _scratch(eng, batch, n, guard=0, fill=0):
    nbytes = eng.square_scratch_bytes(batch, n)
    buf = torch.full((nbytes + 2 * guard + 512,), fill, dtype=torch.uint8, device="cuda")
    base = (buf.data_ptr() + guard + 255) // 256 * 256
    return buf, base, nbytes


def _margin_rows(n):
    rng = np.random.default_rng(n)
    j = np.arange(n + 1, dtype=F32)
    nan_row = 1 - 0.01 * j
    nan_row[[0, 3, n]] = np.nan
    rows = [2 - 0.03 * j,                                              # decreasing, never frozen
            np.ones(n + 1, F32),                                       # constant: nothing is ever accepted
            np.repeat(np.arange((n + 2) // 2, 0, -1, dtype=F32), 2)[:n + 1],          # ties: every second replay repeats
            -0.25 + 0 * j,                                             # crosses zero at replay 0
            np.where(j < n // 2, 1 - 0.01 * j, -0.5),                  # ... in the middle
            np.where(j < n, 1 + 0.01 * j, -1.0),                       # ... at the last replay (rising before: all rejected)
            nan_row,                                                   # NaN at the start, in the middle, at the end
            rng.standard_normal(n + 1).astype(F32) + 1.5]
    return np.stack(rows, 1).astype(F32)


def _logits_for(margin_row, labels, cls, it):
    """Logits whose float32 margin is exactly margin_row: z_y = m, the runner-up 0 (tied between two classes on odd replays),
    everything else negative.  NaN margins: z_y = NaN on even replays, a NaN runner-up on odd ones."""
    B = len(labels)
    z = -1 - np.random.default_rng(it).random((B, cls)).astype(F32)
    for b in range(B):
        y = int(labels[b])
        others = [c for c in range(cls) if c != y]
        z[b, others[it % len(others)]] = 0.0
        if it % 2:
            z[b, others[(it + 3) % len(others)]] = 0.0
        m = margin_row[b]
        if np.isnan(m):
            z[b, y] = np.nan if it % 2 == 0 else 1.0
            if it % 2:
                z[b, others[0]] = np.nan
        else:
            z[b, y] = m
    return z


def _track_all(eng, rows, labels, n, seed, image_offset=0, p_init=0.8):
    """Feeds the rows through the kernel and the reference side by side; returns the kernel's trace_win-equivalent windows."""
    B, cls, S = rows.shape[1], case()["cfg"].num_labels, case()["cfg"].image_size
    eng.plan(B)
    buf, base, nbytes = _scratch(eng, B, n, fill=0xFF)
    sm = R.StateMachine(B, n, S, p_init, seed, image_offset)
    wins = []
    for it in range(n + 1):
        z = _logits_for(rows[it], labels, cls, it)
        want = sm.observe(it, rows[it])
        got = eng.square_track((base, nbytes), B, n, torch.from_numpy(z).cuda(), torch.from_numpy(labels).cuda(), p_init=p_init,
                               seed=seed, image_offset=image_offset, reset=it == 0)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in got.items()}
        assert np.array_equal(got["flags"], want), (it, got["flags"].tolist(), want.tolist())
        assert np.array_equal(got["margin_min"], sm.margin_min), it
        assert np.array_equal(got["queries"], sm.queries), it
        has_p, has_n = (want & P) != 0, (want & N_) != 0
        assert np.array_equal(got["win_prev"][has_p], sm.win_prev[has_p]), it
        assert np.array_equal(got["win_next"][has_n], sm.win_next[has_n]), it
        for b in np.nonzero(has_n)[0]:                      # the windows are the reference's draws
            assert tuple(got["win_next"][b]) == R.proposal(seed, image_offset + b, it + 1, S, sm.side[it + 1]), (it, b)
        wins.append(np.where(has_n[:, None], got["win_next"], -1))
    del buf
    return np.stack(wins)


@pytest.mark.parametrize("n", [10, 50])
def test_square_track_kernel_matches_the_state_machine(n):
    rows = _margin_rows(n)
    labels = np.array([3, 0, 9, 5, 1, 7, 2, 4], np.int64)
    wins = _track_all(engine("f16"), rows, labels, n, seed=7)
    assert (wins[0, 3] == -1).all() and (wins[:, 0, 2] > 0).sum() == n        # frozen at the start / never frozen
    # image_offset: two scratches of 4 images with offsets 0 and 4 draw the windows of one of 8
    lo = _track_all(engine("f16"), rows[:, :4], labels[:4], n, seed=7, image_offset=0)
    hi = _track_all(engine("f16"), rows[:, 4:], labels[4:], n, seed=7, image_offset=4)
    assert np.array_equal(np.concatenate([lo, hi], 1), wins)


def test_square_track_with_another_p_init():
    rows = _margin_rows(10)
    _track_all(engine("f32"), rows, np.array([3, 0, 9, 5, 1, 7, 2, 4], np.int64), 10, seed=2 ** 63 + 5, p_init=0.3)


# ---- 4. the whole attack on its own trace ----------------------------------------------------------------------------------------
def _rebuild(r, x0, n, seed=SEED, image_offset=0, upto=None):
    """x_best as the reference makes it from the margins the GPU saw: the state machine's flags and windows, square_ref.step."""
    S = x0.shape[-1]
    x_cur = R.stripes(x0, EPS, seed, image_offset)
    x_best = x_cur.copy()
    sm = R.StateMachine(x0.shape[0], n, S, 0.8, seed, image_offset)
    tm = r["trace_margin"].numpy()
    for j in range(n + 1 if upto is None else upto):
        flags = sm.observe(j, tm[j])
        x_cur, x_best = R.step(x_cur, x_best, x0, flags, sm.win_prev, sm.win_next, EPS)
    return x_best, sm


@pytest.mark.parametrize("n", [10, 50])
@pytest.mark.parametrize("prec", PRECS)
def test_attack_is_the_state_machine_on_its_own_trace(prec, n):
    c, r = case(), run(prec, n)
    assert r["replays"] == n + 1
    x_best, sm = _rebuild(r, c["x"].numpy(), n)
    assert np.array_equal(r["trace_win"].numpy(), sm.trace_win)               # draws, active and accepted bits
    assert np.array_equal(r["margin_min"].numpy(), sm.margin_min)
    assert np.array_equal(r["queries"].numpy(), sm.queries)
    assert np.array_equal(r["robust"].numpy(), sm.robust)
    assert np.array_equal(r["x_best"].numpy(), x_best)                        # bit for bit
    if n == 50:       # the CPU oracle fools image 4 with proposal 1 (margin -0.069 from 0.076 at the stripes): something is accepted
        assert (r["trace_win"][..., 3] & 16).any(), "no proposal was ever accepted: the case shows nothing"


# ---- 5. invariants ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [10, 50])
@pytest.mark.parametrize("prec", PRECS)
def test_attack_invariants(prec, n):
    c, r, eng = case(), run(prec, n), engine(prec)
    x, y = c["x"], c["y"]
    assert (r["x_best"] - x).abs().max().item() <= EPS + 1e-6
    assert r["x_best"].min().item() >= 0 and r["x_best"].max().item() <= 1
    tm, tw, mm, q = r["trace_margin"], r["trace_win"], r["margin_min"], r["queries"]
    for b in range(8):
        acc = [0] + [j for j in range(1, n + 1) if tw[j - 1, b, 3] & 16]
        seq = tm[acc, b]
        assert (seq[1:] < seq[:-1]).all(), b                                  # margin_min falls along the accepted replays
        assert seq[-1] == mm[b]
        if mm[b] <= 0:                                                        # frozen after replay q - 1: forwarded unchanged
            assert int(q[b]) - 1 == acc[-1]
            assert torch.equal(tm[int(q[b]) - 1:, b], mm[b].expand(n + 2 - int(q[b]))), b
            assert not (tw[int(q[b]) - 1:, b] != 0).any()
        else:
            assert int(q[b]) == n + 1
    assert torch.equal(r["robust"], mm > 0)
    # x_best carries margin_min: re-forwarded at the same batch size
    got, logits = margins(eng, r["x_best"], y)
    err = np.abs(got - mm.numpy()) / np.maximum(1.0, np.abs(mm.numpy()))
    print(f"{prec} N={n}: re-forwarded x_best margin differs from margin_min by at most {err.max():.3e} "
          f"(bit-equal: {np.array_equal(got, mm.numpy())}); robust = {r['robust'].int().tolist()}, margin_min = {mm.tolist()}")
    assert err.max() < TOL_ACT[prec]
    fooled = ~r["robust"]
    assert (logits.argmax(1) != y)[fooled].all()                              # every non-robust image is misclassified at x_best
    if prec == "f32" and n == 50:
        # the float32 CPU oracle with the same draws ends this case with robust = [1,0,1,1,0,0,0,1]: images 1 and 4 fooled at
        # -0.089 / -0.069, images 0, 3, 7 robust at 0.15 / 0.30 / 0.18 (tests/test_square_ref_cpu.py) -- far from any rounding
        assert r["robust"].any() and fooled.any()


# ---- 6. resumable ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_chunks_equal_one_call(prec):
    c, eng, whole = case(), engine(prec), run(prec, 50)
    x, y = c["x"].cuda(), c["y"].cuda()
    eng.square_attack(x, y, EPS, 50, seed=SEED, count=1)                      # make this scratch current; its graph exists
    before = eng.counter("graph_captures")
    first = 0
    for count in (1, 10, 15, 25):
        r = _cpu(eng.square_attack(x, y, EPS, 50, seed=SEED, trace=True, first=first, count=count))
        first += count
        assert r["replays"] == first
        x_best, sm = _rebuild(whole, c["x"].numpy(), 50, upto=first)           # a prefix: the reference rebuilt up to here
        assert np.array_equal(r["x_best"].numpy(), x_best) and np.array_equal(r["margin_min"].numpy(), sm.margin_min)
        assert torch.equal(r["trace_margin"][:first], whole["trace_margin"][:first])
        assert not r["trace_margin"][first:].any()                            # rows of replays that have not run are not written
    assert eng.counter("graph_captures") == before                            # no second graph
    same(whole, r, "chunks")
    with pytest.raises(pkg().VitLoraError):
        eng.square_attack(x, y, EPS, 50, seed=SEED, first=40, count=12)       # 52 > N + 1


def test_check_every_stops_once_no_image_is_active():
    c, eng = case(), engine("f16")
    x = c["x"].cuda()
    wrong = ((c["y"] + 1) % c["cfg"].num_labels).cuda()                       # every margin is negative at the stripes
    r = eng.square_attack(x, wrong, EPS, 50, seed=SEED, check_every=5, trace=True)
    assert r["replays"] == 5 and not r["robust"].any() and (r["queries"] == 1).all()
    assert np.array_equal(r["x_best"].cpu().numpy(), R.stripes(c["x"].numpy(), EPS, SEED))
    assert not r["trace_win"].any()
    # with images that stay active it runs to the end and equals the single call
    full = _cpu(eng.square_attack(x, c["y"].cuda(), EPS, 50, seed=SEED, check_every=7, trace=True))
    same(run("f16", 50), full, "check_every=7")


# ---- 7. graph replay == eager == under the LDS-poison hook -------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_graph_replay_equals_eager_and_the_graph_is_reused(prec):
    c, r = case(), run(prec, 10)
    eng = engine(prec)
    x, y = c["x"].cuda(), c["y"].cuda()
    eng.square_attack(x, y, EPS, 10, seed=SEED)                 # (the engine keeps two scratch tensors: make this key current)
    before = eng.counter("graph_captures")
    again = eng.square_attack(x, y, EPS, 10, seed=SEED, trace=True)
    other_seed = eng.square_attack(x, y, EPS, 10, seed=SEED + 1, trace=True)
    assert eng.counter("graph_captures") == before              # same (batch, eps, N, scratch): nothing new, whatever the seed
    assert not torch.equal(other_seed["trace_win"].cpu(), r["trace_win"])
    os.environ["VITLORA_NO_GRAPH"] = "1"
    try:
        eng2 = make_engine(c["cfg"], c["w"], c["lora"], precision=prec)
        eager = eng2.square_attack(x, y, EPS, 10, seed=SEED, trace=True)
        assert eng2.counter("graph_captures") == 0
    finally:
        os.environ.pop("VITLORA_NO_GRAPH")
    same(r, again, "second call")
    same(r, eager, "eager")
    eng.square_attack(x, y, EPS, 3, seed=SEED)                  # another N is another graph
    assert eng.counter("graph_captures") == before + 1
    eng.set_option("fuse_pgd", 1)                               # a switch changed: the graphs are dropped
    eng.square_attack(x, y, EPS, 10, seed=SEED)
    assert eng.counter("graph_captures") == before + 2


def test_attack_under_the_lds_poison_hook_runs_eagerly_and_equals_the_replay():
    c, r, eng = case(), run("f16", 10), engine("f16")
    n0, g0 = eng.counter("lds_poisons"), eng.counter("graph_captures")
    try:
        eng.set_option("poison_lds", 1)
        got = eng.square_attack(c["x"].cuda(), c["y"].cuda(), EPS, 10, seed=SEED, trace=True)
        torch.cuda.synchronize()
    finally:
        eng.set_option("poison_lds", 0)
    assert eng.counter("lds_poisons") - n0 > 100 and eng.counter("graph_captures") == g0
    same(r, got, "poison_lds")


# ---- 8. scratch contents, guard bands, refusals ----------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_results_do_not_depend_on_the_scratch_and_nothing_outside_it_is_written(prec):
    c, eng = case(), engine(prec)
    n, guard = 10, 1 << 20
    x, y = c["x"].cuda(), c["y"].cuda()
    for fill in (0x00, 0xFF):
        buf, base, nbytes = _scratch(eng, 8, n, guard=guard, fill=0xA5)
        off = base - buf.data_ptr()
        buf[off:off + nbytes] = fill
        for _ in range(2):
            got = eng.square_attack(x, y, EPS, n, seed=SEED, trace=True, scratch=(base, nbytes))
            torch.cuda.synchronize()
            same(run(prec, n), got, f"fill {fill:#x}")
        assert bool((buf[:off] == 0xA5).all()), "bytes BEFORE the scratch were written"
        assert bool((buf[off + nbytes:] == 0xA5).all()), "bytes AFTER the scratch were written"
    E = pkg().VitLoraError
    with pytest.raises(E):                  # one byte short
        eng.square_attack(x, y, EPS, n, scratch=(base, nbytes - 1))
    with pytest.raises(E):                  # unaligned
        eng.square_attack(x, y, EPS, n, scratch=(base + 16, nbytes))
    for kw in (dict(n_queries=0), dict(n_queries=65536), dict(p_init=0.0), dict(p_init=1.5), dict(eps=float("inf")),
               dict(eps=-1.0), dict(first=5, count=7), dict(first=0, count=0)):
        args = dict(eps=EPS, n_queries=n)
        args.update(kw)
        with pytest.raises(E):
            eng.square_attack(x, y, **args)
    eng.check()                             # and none of the refused calls left anything behind
    same(run(prec, n), eng.square_attack(x, y, EPS, n, seed=SEED, trace=True), "after the refusals")


# ---- 9. facade -------------------------------------------------------------------------------------------------------------------
def _model(prec="f16"):
    Pk, c = pkg(), case()
    cfg = c["cfg"]
    arch = Pk.ArchConfig(image_size=cfg.image_size, patch_size=cfg.patch_size, hidden=cfg.hidden, layers=cfg.layers,
                         heads=cfg.heads, mlp=cfg.mlp, num_labels=cfg.num_labels, ln_eps=cfg.ln_eps)
    m = Pk.create_vit_model(cfg.num_labels, arch=arch, precision=prec)
    m.load_state_dict(c["w"])
    return m.eval()


def test_square_normalisation_sandwich_matches_the_engine_sequence():
    Pk, c = pkg(), case()
    model = _model()
    eng = model._engine()
    mean, std = Pk.get_normalization(None)
    y = c["y"].cuda()
    xn = O.normalise(c["x"]).cuda()
    for bad in (dict(norm="L2"), dict(loss="ce"), dict(resc_schedule=False)):
        with pytest.raises(ValueError):
            Pk.Square(model, **bad)
    atk = Pk.Square(Pk.LogitsModel(model), norm="Linf", eps=EPS, n_queries=30, n_restarts=2, seed=7)
    atk.set_normalization_used(mean=mean, std=std)
    got = atk(xn, y)
    # by hand
    eng.set_normalization(mean, std)
    x = eng.channel_affine(xn, std, mean)
    correct = eng.forward(x, normalise=True).argmax(1) == y
    want, robust = x.clone(), correct.clone()
    for r in range(2):
        res = eng.square_attack(x, y, EPS, 30, seed=7 + r)
        take = robust & ~res["robust"]
        want[take] = res["x_best"][take]
        robust &= res["robust"]
    want = eng.channel_affine(want, [1 / s for s in std], [-m / s for m, s in zip(mean, std)])
    assert torch.equal(got, want)
    assert (~robust).any() and torch.equal(atk.last["robust"], res["robust"])
    st = torch.tensor(std).view(1, 3, 1, 1).cuda()
    assert ((got - xn) * st).abs().max().item() <= EPS + 1e-5


def test_autoattack_custom_suite():
    Pk, c = pkg(), case()
    model = _model()
    eng = model._engine()
    x = c["x"].cuda()
    with pytest.raises(NotImplementedError, match="APGD-T, FAB-T and Square"):
        Pk.AutoAttack(model, norm="Linf", eps=EPS, version="standard")
    for bad in (["fab-t"], ["apgd-ce", "apgd-t"], []):
        with pytest.raises(NotImplementedError):
            Pk.AutoAttack(model, norm="Linf", eps=EPS, version="custom", attacks_to_run=bad)
    clean = eng.forward(x, normalise=True).argmax(1).cpu()
    y = clean.clone()
    y[0] = (y[0] + 1) % c["cfg"].num_labels               # image 0 is clean-wrong
    eps = EPS / 8                                         # small enough that APGD-CE with 5 steps leaves images robust
    kw = dict(norm="Linf", eps=eps, version="custom", seed=1, steps=5, square_queries=30)
    a1 = Pk.AutoAttack(model, attacks_to_run=["apgd-ce"], **kw)
    o1 = a1.run_standard_evaluation(x, y.cuda(), bs=8).cpu()
    a2 = Pk.AutoAttack(model, attacks_to_run=["apgd-ce", "square"], **kw)
    o2 = a2.run_standard_evaluation(x, y.cuda(), bs=8).cpu()
    a3 = Pk.AutoAttack(model, attacks_to_run=["square"], **kw)
    o3 = a3.run_standard_evaluation(x, y.cuda(), bs=8).cpu()
    fooled1 = (o1 != c["x"]).flatten(1).any(1)
    assert torch.equal(o2[fooled1], o1[fooled1])          # never un-fools (or moves) an image APGD-CE fooled
    for a, o in ((a1, o1), (a2, o2), (a3, o3)):
        pred = eng.forward(o.cuda(), normalise=True).argmax(1).cpu()
        changed = (o != c["x"]).flatten(1).any(1)
        assert not changed[0]                             # clean-wrong: returned as it was
        assert (pred != y)[changed].all() and (pred == y)[~changed][1:].all()
        assert (o - c["x"]).abs().max().item() <= eps + 1e-6
        assert a.robust_accuracy == float((~changed)[1:].sum()) / 8
    assert a2.robust_accuracy <= a1.robust_accuracy
    print(f"robust accuracy at eps {eps:.4f}: apgd-ce {a1.robust_accuracy}, apgd-ce + square {a2.robust_accuracy}, square {a3.robust_accuracy}")
    # Square draws by the image's index in x_orig: two batches of 4 give what one batch of 8 gives
    o4 = Pk.AutoAttack(model, attacks_to_run=["square"], **kw).run_standard_evaluation(x, y.cuda(), bs=4).cpu()
    same4 = (o4 == o3).flatten(1).all(1)
    print(f"bs=4 against bs=8: {int(same4.sum())} of 8 images bit-equal")
    assert same4[0]


def test_auto_attack_cli_runs_both_components(tmp_path):
    import sys
    from helpers import ROOT
    sys.path.insert(0, ROOT)
    auto_attack = importlib.import_module("auto_attack")
    out = tmp_path / "adv"
    auto_attack.main(["--model", "google_vit", "--source", "gtsrb", "--output_dir", str(out), "--synthetic", "8", "--arch", "tiny",
                      "--num_classes", "10", "--batch_size", "8", "--steps", "5", "--splits", "val", "test",
                      "--attacks", "apgd-ce", "square", "--square_queries", "20", "--check_every", "8"])
    from PIL import Image
    for split in ("val", "test"):
        d = out / "google_vit" / "gtsrb" / split / "auto" / "images"
        names = sorted(os.listdir(d))
        assert names == [f"{split}_{i:06d}.png" for i in range(8)]
        img = Image.open(d / names[0])
        assert img.size == (64, 64) and img.mode == "RGB"
