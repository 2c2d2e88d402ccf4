"""Float64 reference, derived error bounds and element-wise comparator for the attention kernels (CPU only).

tests/test_hip_attn_ref.py hands caller-owned operands to ONE named attention kernel (vl_debug_attention) and compares every
output element with the plain float64 softmax attention of the STORED input values here, and with its textbook backward.
Nothing in this module restates a kernel: no tiles, no online softmax, no fragment maps.  It reuses round16, rnd, sum_bound,
compare_exact and compare_bounded of tests/gemm_ref.py.

Reference (per image and head; q, k, v = the head's 64 columns of the three groups of qkv)
---------
  S = q k^T / 8,  P = softmax(S),  O = P v,  lse = log sum_k exp(S_ik)
  dV = P^T dO,  dP = dO v^T,  delta = rowsum(dO * O),  dS = P * (dP - delta),  dQ = dS k / 8,  dK = dS^T q / 8
  CLS kernels: query row 0 only (compact ctx / dctx rows; dQ of every other token is zero).
  t = ctx Ad^T and u_md = d{q,k,v} Bd_md^T from the float64 ctx / dqkv.
  Unit of lse: the 16-bit kernels keep lse2 = lse / ln 2 (base-2 log-sum-exp of the scaled scores), the fp32 kernels lse.

Operands
--------
uniform      q = 0, k / v / dO on the grid k/8.  Every score is 0, exp2(0) = 1 exactly, l = T exactly, sum_k v_kj is an exact
             grid sum: ctx = (sum_k v_kj) (1/T) and lse2 = log2 T with NO rounding but the ones of 1/l, the product with it and
             log2f (`uniform_forward_allowed`).  The backward on these operands is held to the general bound below (P = 1/T is
             not a 16-bit number unless T is a power of two), with the score terms vanishing because |q| = 0.
permutation  token j carries the code (a, b) = divmod(j, 16): k_j = 32 e_a + 32 e_{16+b}; q_i = the code of pi(i), pi a
             fixed-seed permutation per head.  Raw scores are 2048 for the key pi(i) and at most 1024 for every other key: 184
             units of the base-2 exponent apart (the issue asks for at least 40), so every other probability is below 2^-149 and is
             ZERO in fp32 whatever the type (v_exp_f32 flushes), P = 1 at pi(i).  Hence, with v / dO / Ad / Bd on the grid:
             ctx = v[pi] bit for bit, dV[pi(i)] = dO[i] bit for bit (P = 1 + O(2^-15) rounds to the 16-bit 1), dP - delta is
             the difference of the same exact grid sum = +0, so dQ = dK = +0 exactly; t and u are exact grid sums.
continuous   N(0, 1) operands at full mantissa, q scaled per head so that the scaled scores have standard deviation 1, 2, 3.
peaked       the same plus one feature that shifts the scores: "growing" = +32 (scaled) per 16-key group, so the row maximum
             grows at every tile and the kernels' rescale branch runs at every tile; "first" = +32 on key 0, so the maximum
             sits in tile 0 and the branch never runs again (the random part of a score stays below 6 sigma = 18).  The builders assert both properties on the float64 scores.

Bounds (continuous cases, and lse everywhere)
------
u = 2^-24 (fp32 unit roundoff), U = 2^-23 (one fp32 ulp), h = 16-bit unit roundoff (2^-11 fp16, 2^-8 bf16, 0 on the fp32 path),
a16 = absolute rounding error of a 16-bit value in the subnormal range (2^-25 fp16, 2^-134 bf16, 0 fp32), c = units of the
exponent per raw score (log2(e) / 8 for the 16-bit kernels' exp2, 1/8 for the fp32 kernels' expf), ln = ln 2 resp. 1,
sum_bound(a, K) = 2 (K + 2) u a (gemm_ref: a K-term fp32 sum, doubled for a truncating adder).  Rounding points, from the sources:
  raw score        s_ik: 64-term fp32 sum (MFMA / fma chain + butterfly)            E_s = sum_bound(|q| |k|^T, 64)
  exponent         fma(s, c, -m c): the constant c (u), the product m c (u), the fma (u); the per-tile rescale factor
                   exp2((m_old - m_new) c) (difference, product, constant: 3u on jumps that sum to at most the row range R):
                     Delta_ik = c E_s,ik + (5 R_i + A_i) c u,   A_i = max_k |s_ik| + max_k E_s,ik >= |m|
                   backward (no running maximum, lse is an input with error e_lse: |lse| u for the fp32 image of the float64
                   value, the forward's own bound in a chained case):
                     Delta_ik = c E_s,ik + (|s_ik| c + |t_ik|) u + e_lse,i,   t = s c - lse
  one v_exp_f32    1 ulp (expf / logf of the fp32 kernels: documented 1 ulp, charged 2): Uexp
                   rho_ik = expm1(ln Delta_ik) + Uexp + tiles (Uexp + u)   (the rescale: one exp and one product per tile; forward only)
  l = sum_k p      fp32 over T terms and the rescale products:   rl_i = sum_k P_ik rho_ik + sum_bound(1, T + tiles)
  P -> 16 bit      pack8 / p16: |p16 - P| <= P (rho + h (1 + rho)) + a16 =: eP      (l sums the UNROUNDED p)
  numerator        fp32 over T terms:  eN_ij = sum_k eP_ik |v_kj| + sum_bound(sum_k (P + eP)_ik |v_kj|, T + tiles)
  1 / l, product   U + u:   E_ctx = (eN + |O| (rl + U + u)) / (1 - rl - U - u)
  final rounding   allowed = E + rnd(|O| + E)
  lse              m c (2 A c u: the constant and the product) + log(l) (rl / (1 - rl) / ln, and the function: (|log l| + 2) Ulog,
                   the 2 for its behaviour near l = 1) + the final sum (|lse| u)
  backward         dP: E_dp = sum_bound(|dO| |v|^T, 64);  delta from the STORED 16-bit ctx (error e_ctx = rnd(|O|), or the
                   forward's bound when chained):  E_delta = sum_d |dO| e_ctx + sum_bound(sum_d |dO| (|O| + e_ctx), 64)
                   dS/scale = p (dP - delta), two roundings:  E_ds = P (E_dp + E_delta) (1 + rho) + |dS/scale| (rho + 2u)
                   dS/scale -> 16 bit (pack8 / ds16):          eD = E_ds + h (|dS/scale| + E_ds) + a16
                   dQ = (1/8) sum_k ds16 k (the 1/8 is exact): E = (1/8) (eD |k| + sum_bound((|dS/scale| + eD) |k|, T)), dK likewise
                   with |q| over the queries;  dV = sum_i p16 dO:  E = eP^T |dO| + sum_bound((P + eP)^T |dO|, T)
                   then the final 16-bit rounding.
  t / u            E = allowed(x) |W|^T + sum_bound((|x| + allowed(x)) |W|^T, D + H) (64-term products, fp32 sums over the
                   heads), then one 16-bit rounding; x = ctx resp. dq / dk / dv as stored.
  underflow        v_exp_f32 flushes results below 2^-126 and the fp32 pipes may flush denormal results: every probability carries an
                   absolute error FLUSH = 2^-126 on top of eP (and FLUSH |dP - delta| in dS/scale), every K-term sum (K + 2) FLUSH
                   (`sumb`).  These terms only matter where a peaked case drives P below the fp32 range.
  the reference    float64 sums of T terms cancel to about 2^-53 T of their absolute sum; where a criterion has no summation term
                   of its own (uniform forward) 2^-50 sum_k P |v| is added for it.
Every quantity is float64 and comes from the inputs and the sources, never from a kernel output.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch

import gemm_ref as G
from gemm_ref import compare_bounded, compare_exact, rnd, round16, sum_bound

HD = 64
U24, U23 = 2.0 ** -24, 2.0 ** -23
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
SENTINEL16 = G.SENTINEL16
FLUSH = 2.0 ** -126


def sumb(abs_terms, K):
    """sum_bound of gemm_ref plus the flush-to-zero allowance of a K-term fp32 sum (module docstring: underflow)."""
    return sum_bound(abs_terms, K) + (K + 2) * FLUSH


@dataclass
class Prec:
    dtype: torch.dtype
    h: float          # 16-bit unit roundoff
    a16: float        # absolute error of a 16-bit rounding in the subnormal range
    base2: bool       # lse unit and exponent base
    tile: int         # keys per online-softmax tile
    uexp: float       # exp / log function error


PRECS = {"f16": Prec(torch.float16, 2.0 ** -11, 2.0 ** -25, True, 32, U23),
         "bf16": Prec(torch.bfloat16, 2.0 ** -8, 2.0 ** -134, True, 32, U23),
         "f32": Prec(torch.float32, 0.0, 0.0, False, 16, 2.0 * U23)}


# ---- the case ---------------------------------------------------------------------------------------------------------------
@dataclass
class AttnCase:
    """Stored operand values (CPU tensors of the operand type).  qkv [B*T, 3D]; dO [B*T, D] (CLS: [B, D]);
    Ad [r, D]; Bd [3r, 3D]."""
    kind: str
    B: int
    T: int
    H: int
    qkv: torch.Tensor
    dO: torch.Tensor
    cls: bool = False
    Ad: Optional[torch.Tensor] = None
    Bd: Optional[torch.Tensor] = None
    r: int = 0
    mods: int = 0
    perm: Optional[torch.Tensor] = None        # [H, T] pi of the permutation kind

    @property
    def D(self):
        return HD * self.H


def heads(x, B, T, H):
    """[B*T, H*64] -> float64 [B, H, T, 64]"""
    return x.double().reshape(B, T, H, HD).permute(0, 2, 1, 3)


def rows(x):
    """[B, H, T, 64] -> [B*T, H*64]"""
    B, H, T, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * HD)


def split_qkv(c: AttnCase):
    D = c.D
    q, k, v = (heads(c.qkv[:, i * D:(i + 1) * D], c.B, c.T, c.H) for i in range(3))
    return (q[:, :, :1] if c.cls else q), k, v


def d_out(c: AttnCase):
    return heads(c.dO, c.B, 1 if c.cls else c.T, c.H)


# ---- operand generators -----------------------------------------------------------------------------------------------------
def _down(gen, c: AttnCase, r, mods, dtype, grid):
    if not r:
        return c
    D = c.D
    mk = (lambda s: G.grid(gen, s).to(dtype)) if grid else (lambda s: G.weights(gen, s, dtype))
    c.Ad, c.Bd, c.r, c.mods = mk((r, D)), mk((3 * r, 3 * D)), r, mods
    return c


def uniform_case(B, T, H, prec, seed=0, cls=False, r=0, mods=0):
    gen = torch.Generator().manual_seed(4000 + seed)
    dt, D = DTYPES[prec], HD * H
    qkv = G.grid(gen, (B * T, 3 * D))
    qkv[:, :D] = 0
    dO = G.grid(gen, (B if cls else B * T, D))
    return _down(gen, AttnCase("uniform", B, T, H, qkv.to(dt), dO.to(dt), cls), r, mods, dt, True)


def permutation_case(B, T, H, prec, seed=0, cls=False, r=0, mods=0):
    assert T <= 256
    gen = torch.Generator().manual_seed(5000 + seed)
    dt, D = DTYPES[prec], HD * H
    qkv = G.grid(gen, (B * T, 3 * D)).reshape(B, T, 3, H, HD)
    code = torch.zeros(T, HD, dtype=torch.float64)
    j = torch.arange(T)
    code[j, j // 16] = 32.0
    code[j, 16 + j % 16] = 32.0
    perm = torch.stack([torch.randperm(T, generator=gen) for _ in range(H)])
    for hd in range(H):
        qkv[:, :, 0, hd] = code[perm[hd]]
        qkv[:, :, 1, hd] = code
    dO = G.grid(gen, (B if cls else B * T, D))
    c = AttnCase("permutation", B, T, H, qkv.reshape(B * T, 3 * D).to(dt), dO.to(dt), cls, perm=perm)
    return _down(gen, c, r, mods, dt, True)


def continuous_case(B, T, H, prec, seed=0, cls=False, r=0, mods=0, peak=None):
    """peak: None, "growing" or "first" (module docstring)."""
    gen = torch.Generator().manual_seed(6000 + seed)
    dt, D = DTYPES[prec], HD * H
    x = torch.randn(B, T, 3, H, HD, generator=gen)
    for hd in range(H):
        x[:, :, 0, hd] *= 1.0 + hd % 3                     # scaled scores of standard deviation 1, 2, 3
    if peak:
        x[:, :, 0, :, 0] = 8.0
        x[:, :, 1, :, 0] = 0.0
        if peak == "growing":
            x[:, :, 1, :, 0] = (32.0 * (torch.arange(T) // 16)).view(1, T, 1)
        else:
            x[:, 0, 1, :, 0] = 32.0
    dO = torch.randn(B if cls else B * T, D, generator=gen)
    c = AttnCase("continuous" if not peak else "peaked_" + peak, B, T, H, x.reshape(B * T, 3 * D).to(dt), dO.to(dt), cls)
    if peak:                                               # the property the case is for, on the float64 scores of the stored values
        q, k, _ = split_qkv(c)
        S = q @ k.transpose(-1, -2)
        if peak == "first":
            assert bool((S.argmax(-1) < 16).all())
        else:
            tm = torch.stack([S[..., t0:t0 + 16].max(-1).values for t0 in range(0, T, 16)], -1)
            assert bool((tm[..., 1:] > tm[..., :-1]).all())
    return _down(gen, c, r, mods, dt, False)


BUILDERS = {"uniform": uniform_case, "permutation": permutation_case, "continuous": continuous_case,
            "peaked_growing": lambda *a, **k: continuous_case(*a, peak="growing", **k),
            "peaked_first": lambda *a, **k: continuous_case(*a, peak="first", **k)}


# ---- float64 reference ------------------------------------------------------------------------------------------------------
def reference(c: AttnCase, prec: str) -> dict:
    """Float64 forward and textbook backward of the stored values.  'lse' is in the unit of `prec`'s kernels."""
    p = PRECS[prec]
    q, k, v = split_qkv(c)
    dO = d_out(c)
    Sraw = q @ k.transpose(-1, -2)
    S = Sraw / 8.0
    m = S.max(-1, keepdim=True).values
    w = torch.exp(S - m)
    L = w.sum(-1, keepdim=True)
    P = w / L
    O = P @ v
    lse = (m + torch.log(L)).squeeze(-1)
    dV = P.transpose(-1, -2) @ dO
    dP = dO @ v.transpose(-1, -2)
    delta = (dO * O).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dQ = dS @ k / 8.0
    dK = dS.transpose(-1, -2) @ q / 8.0
    if c.cls:                                              # dQ of the CLS row; zeros for every other token
        full = torch.zeros_like(k)
        full[:, :, :1] = dQ
        dQ = full
    if c.kind == "permutation":
        # the exact statement of the module docstring: float64 leaves terms of relative size e^-128 whose sign would decide
        # between +0 and -0 after rounding; the kernels' fp32 probabilities of the other keys are exactly zero
        Oe, dVe = torch.zeros_like(O), torch.zeros_like(dV)
        for hd in range(c.H):
            pi = c.perm[hd][:q.shape[2]]
            Oe[:, hd] = v[:, hd, pi]
            dVe[:, hd, pi] = dO[:, hd]
        assert float((Oe - O).abs().max()) < 1e-30 and float((dVe - dV).abs().max()) < 1e-30
        assert float(dQ.abs().max()) < 1e-30 and float(dK.abs().max()) < 1e-30
        O, dV, dQ, dK, dS = Oe, dVe, torch.zeros_like(dQ), torch.zeros_like(dK), torch.zeros_like(dS)
    out = dict(q=q, k=k, v=v, dO=dO, Sraw=Sraw, P=P, L=L, O=O, lse_nat=lse, lse=lse / LN2 if p.base2 else lse,
               dP=dP, delta=delta, dSp=dS, dq=dQ + 0.0, dk=dK + 0.0, dv=dV + 0.0)
    out["ctx2d"] = rows(O)
    out["lse2d"] = out["lse"].reshape(c.B * c.H, -1)
    for n in ("dq", "dk", "dv"):
        out[n + "2d"] = rows(out[n])
    if c.Ad is not None and not c.cls:
        t = torch.zeros(c.B * c.T, 64, dtype=torch.float64)
        t[:, :c.r] = out["ctx2d"] @ c.Ad.double().T
        out["t2d"] = t + 0.0
        u = torch.zeros(c.B * c.T, 64, dtype=torch.float64)
        D = c.D
        for md, n in enumerate(("dq", "dk", "dv")):
            if (c.mods >> md) & 1:
                u[:, md * c.r:(md + 1) * c.r] = out[n + "2d"] @ c.Bd.double()[md * c.r:(md + 1) * c.r, md * D:(md + 1) * D].T
        out["u2d"] = u + 0.0
    return out


# ---- bounds -----------------------------------------------------------------------------------------------------------------
def _c(p: Prec):
    return (LOG2E / 8.0, LN2) if p.base2 else (0.125, 1.0)


STRUCTURED = ("uniform", "permutation")


def _score_bound(c, q, k):
    """E_s; zero for the structured kinds, whose raw scores are exact fp32 sums (0, or multiples of 1024 up to 2048)."""
    ab = q.abs() @ k.abs().transpose(-1, -2)
    if c.kind in STRUCTURED:
        G.exact_guard(ab, 1024.0)
        return torch.zeros_like(ab)
    return sumb(ab, HD)


def forward_allowed(c: AttnCase, ref: dict, prec: str) -> dict:
    """allowed error of 'ctx' [B*T, D] and 'lse' [B*H, Tq] (module docstring)."""
    p = PRECS[prec]
    cc, ln = _c(p)
    q, k, v, Sraw, P, O = (ref[n] for n in ("q", "k", "v", "Sraw", "P", "O"))
    T = c.T
    tiles = -(-T // p.tile)
    E_s = _score_bound(c, q, k)
    R = Sraw.max(-1, keepdim=True).values - Sraw.min(-1, keepdim=True).values
    A = Sraw.abs().max(-1, keepdim=True).values + E_s.max(-1, keepdim=True).values
    Delta = cc * E_s + (5.0 * R + A) * cc * U24
    rho = torch.expm1(ln * Delta) + p.uexp + tiles * (p.uexp + U24)
    rl = (P * rho).sum(-1, keepdim=True) + float(sum_bound(torch.tensor(1.0), T + tiles)) + (T + 2) * FLUSH
    eP = P * (rho + p.h * (1.0 + rho)) + p.a16 + FLUSH
    eN = eP @ v.abs() + sumb((P + eP) @ v.abs(), T + tiles)
    one = rl + U23 + U24
    E = (eN + O.abs() * one) / (1.0 - one)
    lse = ref["lse"].unsqueeze(-1)
    logl = torch.log(ref["L"]) / ln
    E_lse = 2.0 * A * cc * U24 + rl / (1.0 - rl) / ln + (logl.abs() + 2.0) * p.uexp + lse.abs() * U24
    E2, O2 = rows(E), rows(O)
    return dict(ctx=E2 + rnd(O2.abs() + E2, p.dtype), lse=E_lse.reshape(c.B * c.H, -1))


def uniform_forward_allowed(c: AttnCase, ref: dict, prec: str) -> dict:
    """Uniform case: only 1/l (U), the product with it (u), log2f ((log2 T + 2) U) and the final roundings are charged."""
    assert c.kind == "uniform"
    p = PRECS[prec]
    v = ref["v"]
    G.exact_guard(v.abs().sum(-2), 2.0 ** -3)              # sum_k v_kj: an exact fp32 sum in any order
    O2 = ref["ctx2d"]
    noise = 2.0 ** -50 * v.abs().mean(-2, keepdim=True).expand(-1, -1, ref["O"].shape[2], -1)     # the float64 reference's own
    E = O2.abs() * (U23 + U24) / (1.0 - U23 - U24) + rows(noise)
    lse = ref["lse2d"]
    E_lse = (lse.abs() + 2.0) * p.uexp + lse.abs() * U24
    return dict(ctx=E + rnd(O2.abs() + E, p.dtype), lse=E_lse)


def backward_allowed(c: AttnCase, ref: dict, prec: str, lse_err=None, ctx_err=None) -> dict:
    """allowed error of 'dq', 'dk', 'dv' [B*T, D].  lse_err [B, H, Tq, 1] / ctx_err [B, H, Tq, 64]: error of the lse / ctx the
    kernel is GIVEN against the float64 ones (default: their fp32 / 16-bit images; chained cases pass the forward's bounds)."""
    p = PRECS[prec]
    cc, ln = _c(p)
    q, k, v, dO, Sraw, P, O, dSp = (ref[n] for n in ("q", "k", "v", "dO", "Sraw", "P", "O", "dSp"))
    T = c.T
    lse = ref["lse"].unsqueeze(-1)
    if lse_err is None:
        lse_err = lse.abs() * U24
    if ctx_err is None:
        ctx_err = rnd(O.abs(), p.dtype) if p.h else O.abs() * U24
    E_s = _score_bound(c, q, k)
    t = Sraw * cc - lse
    Delta = cc * E_s + (Sraw.abs() * cc + t.abs()) * U24 + lse_err
    rho = torch.expm1(ln * Delta) + p.uexp
    E_dp = sumb(dO.abs() @ v.abs().transpose(-1, -2), HD)
    if c.kind in STRUCTURED:                               # grid dO and v: an exact fp32 sum
        G.exact_guard(dO.abs() @ v.abs().transpose(-1, -2), 2.0 ** -6)
        E_dp = torch.zeros_like(E_dp)
    E_delta = (dO.abs() * ctx_err).sum(-1, keepdim=True) + sumb((dO.abs() * (O.abs() + ctx_err)).sum(-1, keepdim=True), HD)
    E_ds = P * (E_dp + E_delta) * (1.0 + rho) + dSp.abs() * (rho + 2.0 * U24) + FLUSH * ((ref["dP"] - ref["delta"]).abs() + E_dp + E_delta + 1.0)
    eD = E_ds + p.h * (dSp.abs() + E_ds) + p.a16
    eP = P * (rho + p.h * (1.0 + rho)) + p.a16 + FLUSH
    Tq = q.shape[2]
    E_dq = 0.125 * (eD @ k.abs() + sumb((dSp.abs() + eD) @ k.abs(), T))
    E_dk = 0.125 * (eD.transpose(-1, -2) @ q.abs() + sumb((dSp.abs() + eD).transpose(-1, -2) @ q.abs(), Tq))
    E_dv = eP.transpose(-1, -2) @ dO.abs() + sumb((P + eP).transpose(-1, -2) @ dO.abs(), Tq)
    if c.cls:
        full = torch.zeros_like(k)
        full[:, :, :1] = E_dq
        E_dq = full
    out = {}
    for n, E in (("dq", E_dq), ("dk", E_dk), ("dv", E_dv)):
        E2 = rows(E)
        out[n] = E2 + rnd(ref[n + "2d"].abs() + E2, p.dtype)
    return out


def down_allowed(x_ref2d, x_allowed, W, ref_out, prec, H):
    """t / u columns of one module: x [B*T, D] (float64 reference, its allowed error), W [r, D] -> [B*T, r]."""
    p = PRECS[prec]
    Wa = W.double().abs()
    E = x_allowed @ Wa.T + sumb((x_ref2d.abs() + x_allowed) @ Wa.T, HD * H + H)
    return E + rnd(ref_out.abs() + E, p.dtype)


def t_allowed(c, ref, allowed_ctx, prec):
    a = torch.zeros(c.B * c.T, 64, dtype=torch.float64)
    a[:, :c.r] = down_allowed(ref["ctx2d"], allowed_ctx, c.Ad, ref["t2d"][:, :c.r], prec, c.H)
    return a


def u_allowed(c, ref, allowed_bwd, prec):
    a = torch.zeros(c.B * c.T, 64, dtype=torch.float64)
    D = c.D
    for md, n in enumerate(("dq", "dk", "dv")):
        if (c.mods >> md) & 1:
            s = slice(md * c.r, (md + 1) * c.r)
            a[:, s] = down_allowed(ref[n + "2d"], allowed_bwd[n], c.Bd[s, md * D:(md + 1) * D], ref["u2d"][:, s], prec, c.H)
    return a


# ---- criteria: what each output of a case is held to ------------------------------------------------------------------------
def expectations(c: AttnCase, ref: dict, prec: str, direction: str, chained: Optional[dict] = None) -> dict:
    """name -> (float64 reference [rows, cols], allowed [rows, cols] or None for bit-exact, criterion name).
    direction 'fwd': ctx, lse (+ t); 'bwd': dq, dk, dv (+ u).  chained: the forward's allowed dict when the backward was
    fed the kernel's own forward outputs."""
    p = PRECS[prec]
    exp = {}
    exact = c.kind == "permutation"
    if direction == "fwd":
        # (the fp32 scalar kernel multiplies every probability with 1/l before the sum: the general bound holds there)
        tight = c.kind == "uniform" and p.h > 0
        fa = uniform_forward_allowed(c, ref, prec) if tight else forward_allowed(c, ref, prec)
        crit = "uniform" if tight else "continuous"
        exp["ctx"] = (ref["ctx2d"], None, "exact") if exact else (ref["ctx2d"], fa["ctx"], crit)
        exp["lse"] = (ref["lse2d"], forward_allowed(c, ref, prec)["lse"] if exact else fa["lse"], "lse")
        if c.Ad is not None and not c.cls:
            exp["t"] = (ref["t2d"], None, "exact") if exact else (ref["t2d"], t_allowed(c, ref, fa["ctx"], prec), crit + "-t")
        return exp
    if exact and chained is None:
        for n in ("dq", "dk", "dv"):
            exp[n] = (ref[n + "2d"], None, "exact")
        if c.Bd is not None and not c.cls:
            exp["u"] = (ref["u2d"], None, "exact")
        return exp
    kw = {}
    if chained is not None:
        kw = dict(lse_err=chained["lse"].reshape(c.B, c.H, -1, 1), ctx_err=heads(chained["ctx"], c.B, 1 if c.cls else c.T, c.H))
    ba = backward_allowed(c, ref, prec, **kw)
    crit = ("chained" if chained is not None else "uniform-bwd" if c.kind == "uniform" else "continuous")
    for n in ("dq", "dk", "dv"):
        exp[n] = (ref[n + "2d"], ba[n], crit)
    if c.Bd is not None and not c.cls:
        exp["u"] = (ref["u2d"], u_allowed(c, ref, ba, prec), crit + "-u")
    return exp


def backward_inputs(c: AttnCase, ref: dict, prec: str):
    """What a backward case is GIVEN: ctx rounded to the operand type, lse as the fp32 of the float64 value."""
    p = PRECS[prec]
    return ref["ctx2d"].float().to(p.dtype), ref["lse2d"].float()


def locate(where, T, lse=False):
    """(row, col, ...) of a 2-D output -> (image, head, token, column); lse rows are (image, head), its columns tokens."""
    out = []
    for w in where:
        r, col = w[0], w[1]
        out.append((r // T, col // HD, r % T, col % HD) if not lse else ("bh", r, col, None))
    return out


def verify(c: AttnCase, got: dict, exp: dict, prec: str):
    """Compares every element of every expected output.  Returns (failures, ratios): failures = [(name, count,
    [(image, head, token, column), ...])], ratios = {(name, criterion): largest error / allowed}."""
    p = PRECS[prec]
    fails, ratios = [], {}
    for name, (ref64, allowed, crit) in exp.items():
        g = got[name]
        assert tuple(g.shape) == tuple(ref64.shape), (name, g.shape, ref64.shape)
        is_lse = name == "lse"
        Trow = 1 if (c.cls and name == "ctx") else c.T
        if allowed is None:
            # the CLS backward's dk / dv are SINGLE products (one query): 0 * x keeps the sign of x, where the sums of every other
            # kernel start at +0 -- their zeros are compared by value
            n, where = compare_exact(g, ref64, g.dtype, signed_zero=not (c.cls and name in ("dk", "dv")))
        else:
            n, where, ratio = compare_bounded(g, ref64, allowed)
            ratios[(name, crit)] = ratio
        if n:
            fails.append((name, n, [(w[0] // c.H, w[0] % c.H, w[1], None) for w in where] if is_lse else locate(where, Trow)))
    return fails, ratios


# ---- a float64 evaluation that rounds where the kernels round, with optional faults (tests/test_attn_ref_cpu.py) ------------
FAULTS_FWD = ["key_T_valid", "last_key_dropped", "key_pair_swapped", "heads_exchanged", "lse_wrong_base", "lse_row_stale",
              "row_unwritten", "t_misses_a_head"]
FAULTS_BWD = ["key_T_valid", "last_key_dropped", "key_pair_swapped", "heads_exchanged", "dq_without_scale", "dk_without_scale",
              "delta_missing", "row_unwritten", "cls_dq_not_zeroed", "u_kv_exchanged"]


def _r16(x, p: Prec):
    return round16(x, p.dtype).double()


def _sentinel(p: Prec):
    if not p.h:
        return float("nan")
    return float(torch.tensor([SENTINEL16], dtype=torch.int16).view(p.dtype).double())


def _pair(T):
    """two keys of the first 32-row tile, in different 16-row halves where T allows"""
    return 0, min(17, T - 1)


def emulate_forward(c: AttnCase, prec: str, fault=None) -> dict:
    p = PRECS[prec]
    cc, ln = _c(p)
    q, k, v = split_qkv(c)
    T = c.T
    if fault == "key_T_valid":                             # the staging loads put row T - 1 into the padding rows
        k, v = torch.cat([k, k[:, :, -1:]], 2), torch.cat([v, v[:, :, -1:]], 2)
    elif fault == "last_key_dropped":
        k, v = k[:, :, :-1], v[:, :, :-1]
    elif fault == "key_pair_swapped":
        a, b = _pair(T)
        v = v.clone()
        v[:, :, [a, b]] = v[:, :, [b, a]]
    s = (q @ k.transpose(-1, -2)).float().double()
    m = s.max(-1, keepdim=True).values
    w = torch.exp(ln * (s - m) * cc).float().double()
    l = w.sum(-1, keepdim=True)
    o = _r16(_r16(w, p) @ v / l, p)
    lse = (m * cc + torch.log(l) / ln).squeeze(-1)
    if fault == "heads_exchanged":
        o[:, [0, 1]], lse[:, [0, 1]] = o[:, [1, 0]], lse[:, [1, 0]]
    if fault == "lse_wrong_base":
        lse = lse * LN2 if p.base2 else lse / LN2
    if fault == "lse_row_stale":                           # one entry keeps what an earlier launch left there: its neighbour's value
        j = lse.shape[-1] // 2
        lse[0, -1, j] = lse[0, -1, j - 1] if j else lse[0, 0, j]
    ctx = rows(o)
    out = dict(lse=lse.reshape(c.B * c.H, -1).float())
    if c.Ad is not None and not c.cls:
        Ad = c.Ad.double().clone()
        if fault == "t_misses_a_head":
            Ad[:, -HD:] = 0
        t = torch.zeros(c.B * T, 64, dtype=torch.float64)
        t[:, :c.r] = ctx @ Ad.T
        out["t"] = _r16(t, p).to(p.dtype)
    if fault == "row_unwritten":
        ctx[ctx.shape[0] // 2] = _sentinel(p)
    out["ctx"] = ctx.to(p.dtype)
    return out


def emulate_backward(c: AttnCase, prec: str, ctx_in, lse_in, fault=None) -> dict:
    """ctx_in / lse_in: what the kernel is given (backward_inputs, or a forward's outputs)."""
    p = PRECS[prec]
    cc, ln = _c(p)
    q, k, v = split_qkv(c)
    dO = d_out(c)
    T, Tq = c.T, q.shape[2]
    O = heads(ctx_in, c.B, Tq, c.H)
    lse = lse_in.double().reshape(c.B, c.H, Tq, 1)
    kx, vx = k, v
    if fault == "key_T_valid":
        kx, vx = torch.cat([k, k[:, :, -1:]], 2), torch.cat([v, v[:, :, -1:]], 2)
    s = (q @ kx.transpose(-1, -2)).float().double()
    P = torch.exp(ln * (s * cc - lse)).float().double()
    dP = (dO @ vx.transpose(-1, -2)).float().double()
    delta = (dO * O).sum(-1, keepdim=True).float().double()
    if fault == "delta_missing":
        delta = torch.zeros_like(delta)
    ds16 = _r16(P * (dP - delta), p)
    p16 = _r16(P, p)
    if fault == "last_key_dropped":
        ds16, p16 = ds16.clone(), p16.clone()
        ds16[..., -1] = 0
        p16[..., -1] = 0
    dq = ds16 @ kx * (1.0 if fault == "dq_without_scale" else 0.125)
    dk = (ds16.transpose(-1, -2) @ q)[:, :, :T] * (1.0 if fault == "dk_without_scale" else 0.125)
    dv = (p16.transpose(-1, -2) @ dO)[:, :, :T]
    if c.cls:
        full = torch.zeros_like(k)
        if fault == "cls_dq_not_zeroed":
            full[:] = _sentinel(p)
        full[:, :, :1] = dq
        dq = full
    if fault == "key_pair_swapped":
        a, b = _pair(T)
        dk[:, :, [a, b]], dv[:, :, [a, b]] = dk[:, :, [b, a]], dv[:, :, [b, a]]
    outs = dict(dq=_r16(dq, p), dk=_r16(dk, p), dv=_r16(dv, p))
    if fault == "heads_exchanged":
        for n in outs:
            outs[n][:, [0, 1]] = outs[n][:, [1, 0]]
    out = {n: rows(x) for n, x in outs.items()}
    if c.Bd is not None and not c.cls:
        D = c.D
        u = torch.zeros(c.B * T, 64, dtype=torch.float64)
        for md, n in enumerate(("dq", "dk", "dv")):
            if (c.mods >> md) & 1:
                src = md if fault != "u_kv_exchanged" or md == 0 else 3 - md
                u[:, src * c.r:(src + 1) * c.r] = out[n] @ c.Bd.double()[md * c.r:(md + 1) * c.r, md * D:(md + 1) * D].T
        out["u"] = _r16(u, p).to(p.dtype)
    if fault == "row_unwritten":
        for n in ("dq", "dk", "dv"):
            out[n][out[n].shape[0] // 2] = _sentinel(p)
    for n in ("dq", "dk", "dv"):
        out[n] = out[n].to(p.dtype)
    return out
