"""Float64 reference and element-wise comparator for the GEMM kernels and their fused epilogues (CPU only).

tests/test_hip_gemm_ref.py hands caller-owned operands to ONE chosen kernel with ONE chosen epilogue (vl_debug_gemm) and
compares every output element with the float64 evaluation of the same product here.  Nothing in this module restates a
kernel: the product is torch's float64 matmul of the STORED 16-bit values, the epilogues are written from their
documentation in csrc/gemm.h, the index maps of the patch epilogues are reshapes / Python loops.

Operands
--------
grid        k/8 with integer k in [-8, 8] (times a power of two where a case scales them).  Every product is a multiple of
            1/64, every partial sum of up to 2^18 such terms a multiple of 1/64 below 2^24/64: exact in fp32 in ANY order and
            on any adder.  The accumulator must therefore EQUAL the float64 sum, and the only rounding left is the one
            conversion to the output type (round to nearest even: common.h f2h).  `exact_guard` asserts the premise for the
            operands actually used: (sum of |terms|) / granularity < 2^24.
continuous  N(0, 1) activations against N(0, 0.05^2) weights at full mantissa: grid values carry three mantissa bits and
            cannot see an operand whose low bits are lost.

Criteria
--------
grid, linear epilogue       got == ref.to(dtype) bit for bit (signed zeros included; compare_exact names the one exception), no slack.
continuous                  |got - ref| <= E + rnd(|ref| + E),
                            E = 2 (K1 + K2 + 2) 2^-24 (|A1| |W1|^T + |A2| |W2|^T + |bias| + |R|): the standard forward bound of
                            a length-K fp32 sum (gamma_K ~ K u, u = 2^-24) doubled to allow a truncating adder;
                            rnd(v) = half a 16-bit ulp of v, bounded from above by 2^-11 v (fp16, floor 2^-25 in the subnormal
                            range) / 2^-8 v (bf16); 0 for fp32 outputs.
                            Epilogues that MULTIPLY the sum scale E by that factor (this module's reasoning, the sum formula
                            does not cover them): EPI_GELU_BWD by |R| (R is then no term of the sum), EPI_DROP_ACC by
                            |G| and its z part by 1/(1-p); two more fp32 roundings are covered by the "+ 2" of (K + 2).
GELU / GELU' on grid z      z is exact, so only the function approximation and one 16-bit rounding remain:
                            |got - ref| <= approx(z) + rnd(|ref| + approx(z)).

approx(z), derived from csrc/gemm_epi.h (gelu_parts), U = 2^-23 = one fp32 ulp (relative), every operation charged a full ulp:
  ax   = |z| c, c = fl(1/sqrt 2)                         rel <= 2U
  d    = fma(0.3275911, ax, 1) in [1, 2.4]               rel <= 3U;   t = v_rcp(d) (1 ulp)  rel <= 4U,  t in (0, 1]
  e    = v_exp(-(ax ax) log2e) (1 ulp): the argument has rel error <= 5U (two roundings of ax^2, the constant, the product),
         i.e. absolute error 5U (z^2/2) log2e, which the exponential turns into rel 2.5 z^2 U; with the v_exp ulp:
         rel(e) <= (3 z^2 + 1) U,  e = exp(-z^2/2)
  poly = 4 fmas on values <= 1.5 (<= 6U absolute) + |poly'(t)| <= 11.73 times the error 4U of t  ->  <= 53U absolute
  q    = poly t e (two products, <= 2U rel more): |q - q_true| <= e (53U + 3U) + q rel(e) <= e (57 + 3 z^2) U   (q <= e)
  erf  = 1 - q (1 ulp of a value <= 1) and Abramowitz-Stegun 7.1.26 itself (|error| <= 1.5e-7, gemm_epi.h):
         d_erf(z) = 1.5e-7 + U + e (57 + 3 z^2) U
  cdf  = 0.5 (1 + erf): one more rounding of a value <= 2:     d_cdf = 0.5 (d_erf + 2U)
  pdf  = fl(1/sqrt(2 pi)) e:                                   d_pdf = pdf ((3 z^2 + 1) U + 2U)
  gelu  = z cdf (one rounding):                                approx = |z| d_cdf + |gelu| U
  gelu' = fma(z, pdf, cdf) (one rounding):                     approx = |z| d_pdf + d_cdf + |gelu'| U
These come from the source, not from any output of the kernel.
"""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

EPI = {"store_h16": 0, "resid_f32": 1, "gelu": 2, "gelu_bwd": 3, "patch_fwd": 4, "patch_bwd": 5, "store_f32": 6,
       "drop_acc": 8, "patch_pgd": 9, "resid_h16": 10}
F32_OUT = {"resid_f32", "store_f32", "patch_bwd", "patch_pgd"}
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
SENTINEL16 = 0x4D3B          # int16 pattern of untouched 16-bit output (fp16 20.92.., bf16 1.96e8: neither is on the grid)
U32 = 2.0 ** -23


# ---- operand generators ---------------------------------------------------------------------------------------------------
def grid(gen, shape, dtype=torch.float32, scale=1.0):
    """k/8, k integer in [-8, 8], times `scale` (a power of two), stored as `dtype`."""
    return (torch.randint(-8, 9, tuple(shape), generator=gen).double() / 8.0 * scale).to(dtype)


def activations(gen, shape, dtype):
    return torch.randn(tuple(shape), generator=gen).to(dtype)


def weights(gen, shape, dtype):
    return (0.05 * torch.randn(tuple(shape), generator=gen)).to(dtype)


# ---- dropout mask of EPI_DROP_ACC, restated from csrc/common.h in Python integers -----------------------------------------
_M64 = (1 << 64) - 1


def mix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def inv_keep32(p: float) -> float:
    """1 / (1 - p) as the fp32 argument the kernel multiplies with."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def drop_keep(seed: int, stream: int, idx: int, p: float) -> bool:
    """Element idx is kept when its 24-bit uniform u = (r >> 40) / 2^24 satisfies u >= p (p as fp32)."""
    r = mix64(((seed * 0xD1342543DE82EF95) & _M64) ^ ((stream << 48) & _M64) ^ idx)
    return (r >> 40) >= float(np.float32(p)) * 16777216.0


def drop_mask(seed: int, stream: int, M: int, N: int, p: float) -> torch.Tensor:
    """[M, N] float64 mask with values 0 or 1/(1-p); element (m, n) has index m * N + n.  Vectorised on uint64 (wrap-around),
    checked against the integer form above by the CPU tests."""
    with np.errstate(over="ignore"):
        idx = np.arange(M * N, dtype=np.uint64)
        z = np.uint64((seed * 0xD1342543DE82EF95) & _M64) ^ np.uint64((stream << 48) & _M64) ^ idx
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    keep = (z >> np.uint64(40)).astype(np.float64) >= float(np.float32(p)) * 16777216.0
    return torch.from_numpy(np.where(keep, inv_keep32(p), 0.0)).reshape(M, N)


# ---- the case -------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """Logical (unpadded) CPU tensors holding the STORED values (16-bit tensors for 16-bit operands)."""
    epi: str
    A1: torch.Tensor                      # [rows, K1]  (a_gather: [B * tokens, K1])
    W1: torch.Tensor                      # [N, K1]
    A2: Optional[torch.Tensor] = None     # [M, K2]
    W2: Optional[torch.Tensor] = None     # [N, K2]
    bias: Optional[torch.Tensor] = None   # [N] fp32
    R: Optional[torch.Tensor] = None      # [M, N] (image layout for patch_pgd: x0)
    G: Optional[torch.Tensor] = None
    M: int = 0                            # rows computed (0: A1's)
    Mvalid: int = 0
    # patch geometry
    pos: Optional[torch.Tensor] = None    # [tokens, N] fp32
    patches: int = 0
    psize: int = 0
    inv_std: tuple = (1.0, 1.0, 1.0)
    row_scale: Optional[torch.Tensor] = None
    a_gather: bool = False
    adv: Optional[torch.Tensor] = None    # patch_pgd: the image being updated [B, 3, img, img]
    pgd: tuple = (0.0, 0.0, 0.0, 1.0)     # eps, alpha, lo, hi
    # dropout
    drop: tuple = (0, 0, 0.0)             # seed, stream, p
    # fused down projection
    down_W: Optional[torch.Tensor] = None  # [64, K1]
    down_cols: int = 64                    # columns of t the kernel computes (16 * down_groups; 64 for the streaming kernel)
    ones_col: bool = False
    extra: dict = field(default_factory=dict)


def _d(t):
    return None if t is None else t.double()


def gather_rows(M: int, Mvalid: int, patches: int):
    """GEMM row m = b * patches + p reads token row b * (patches + 1) + 1 + p; rows past Mvalid read row 0 (never stored)."""
    rows = []
    for m in range(M):
        if m < Mvalid:
            b, p = divmod(m, patches)
            rows.append(b * (patches + 1) + 1 + p)
        else:
            rows.append(0)
    return torch.tensor(rows)


def exact_guard(abs_sum: torch.Tensor, granularity: float):
    """Premise of the bit-exact criteria: every partial sum, in any order, is a multiple of `granularity` of magnitude at most
    abs_sum, hence exact in fp32 when abs_sum / granularity < 2^24."""
    assert float(abs_sum.max()) / granularity < 2.0 ** 24, "grid case outside the exactly representable range"


def round16(x64: torch.Tensor, dtype) -> torch.Tensor:
    """One rounding to nearest even from a value that fp32 holds exactly (float64 -> fp32 is then exact)."""
    return x64.float().to(dtype)


def reference(c: Case, dtype) -> dict:
    """Float64 outputs of the case: 'C' (row layout, token layout for patch_fwd, image layout for patch_bwd / patch_pgd),
    'C2' (gelu'), 't' (fused down projection, rounded to `dtype`), 'z' (sum + bias), 'abs_z' (|A||W|^T + |bias|, row layout:
    the premise of exact_guard), 'abs' (the same in the layout of C and with the epilogue's terms and factors, for E),
    'g' (patch gradient before the PGD step)."""
    M = c.M or c.A1.shape[0]
    Mvalid = c.Mvalid or M
    A1 = _d(c.A1)
    if c.a_gather:
        A1 = A1[gather_rows(M, Mvalid, c.patches)]
    A1 = A1[:M]
    W1 = _d(c.W1)
    z = A1 @ W1.T
    ab = A1.abs() @ W1.abs().T
    out = {}
    A2 = _d(c.A2)
    if c.down_W is not None:
        dw = _d(c.down_W)[:c.down_cols]
        t = round16(A1 @ dw.T + 0.0, dtype)                              # the kernel multiplies the ROUNDED t
        out["t"] = t.double()
        A2 = torch.zeros(M, 64, dtype=torch.float64)
        A2[:, :c.down_cols] = out["t"]
        if c.ones_col:
            A2[:, 63] = 1.0                                        # column 63 of W2 is the bias
    if c.W2 is not None:
        z = z + A2[:M] @ _d(c.W2).T
        ab = ab + A2[:M].abs() @ _d(c.W2).abs().T
    z = z + 0.0                      # the fp32 accumulator starts at +0: a sum that cancels exactly (or of -0 products) is +0
    if c.bias is not None:
        z = z + _d(c.bias)[None, :]
        ab = ab + _d(c.bias).abs()[None, :]
    out["z"], out["abs"], out["abs_z"] = z, ab, ab
    e = c.epi
    if e in ("store_h16", "store_f32"):
        out["C"] = z
    elif e in ("resid_f32", "resid_h16"):
        out["C"] = z + _d(c.R)
        out["abs"] = ab + _d(c.R).abs()
    elif e == "gelu":
        cdf = 0.5 * (1.0 + torch.special.erf(z / np.sqrt(2.0)))
        pdf = torch.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)
        out["C"], out["C2"] = z * cdf, cdf + z * pdf
    elif e == "gelu_bwd":
        out["C"] = z * _d(c.R)
        out["abs"] = ab * _d(c.R).abs()
    elif e == "drop_acc":
        seed, stream, p = c.drop
        mask = drop_mask(seed, stream, M, z.shape[1], p)
        v = _d(c.R) + mask * z
        a = _d(c.R).abs() + mask * ab
        if c.G is not None:
            v, a = v * _d(c.G), a * _d(c.G).abs()
        out["C"], out["abs"], out["mask"] = v, a, mask
    elif e == "patch_fwd":
        B, T = Mvalid // c.patches, c.patches + 1
        N = z.shape[1]
        C = torch.full((B * T, N), float("nan"), dtype=torch.float64)          # NaN: rows the epilogue does not write (CLS)
        A = torch.full((B * T, N), float("nan"), dtype=torch.float64)
        for m in range(Mvalid):
            b, p = divmod(m, c.patches)
            C[b * T + 1 + p] = z[m] + _d(c.pos)[1 + p]
            A[b * T + 1 + p] = ab[m] + _d(c.pos)[1 + p].abs()
        out["C"], out["abs"] = C, A
    elif e in ("patch_bwd", "patch_pgd"):
        B, ps = Mvalid // c.patches, c.psize
        g = int(round(c.patches ** 0.5))
        assert g * g == c.patches and z.shape[1] == 3 * ps * ps
        scale = torch.tensor(c.inv_std, dtype=torch.float64).view(1, 3, 1, 1)
        if c.row_scale is not None:
            scale = scale * _d(c.row_scale)[:B].view(B, 1, 1, 1)

        def to_image(x):          # [b, py, px, ch, ph, pw] -> [b, ch, py * ps + ph, px * ps + pw]
            return x[:Mvalid].reshape(B, g, g, 3, ps, ps).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, g * ps, g * ps)
        grad = to_image(z) * scale
        out["g"], out["abs"] = grad, to_image(ab) * scale.abs()
        if e == "patch_bwd":
            out["C"] = grad
        else:
            eps, alpha, lo, hi = c.pgd
            x0, adv = _d(c.R), _d(c.adv)
            step = (adv + alpha * torch.sign(grad) - x0).clamp(-eps, eps)
            out["C"] = (x0 + step).clamp(lo, hi)
            out["C_plus"] = (x0 + (adv + alpha - x0).clamp(-eps, eps)).clamp(lo, hi)       # outcome of either sign,
            out["C_minus"] = (x0 + (adv - alpha - x0).clamp(-eps, eps)).clamp(lo, hi)      # for |g| below its error bound
    else:
        raise ValueError(e)
    return out


# ---- bounds ---------------------------------------------------------------------------------------------------------------
def rnd(v: torch.Tensor, dtype) -> torch.Tensor:
    """Half a 16-bit ulp of v (from above); zero for fp32 outputs."""
    if dtype == torch.float16:
        return (v * 2.0 ** -11).clamp_min(2.0 ** -25)
    if dtype == torch.bfloat16:
        return v * 2.0 ** -8
    return torch.zeros_like(v)


def sum_bound(abs_terms: torch.Tensor, K: int) -> torch.Tensor:
    """E of the module docstring."""
    return 2.0 * (K + 2) * 2.0 ** -24 * abs_terms


def continuous_allowed(ref: torch.Tensor, abs_terms: torch.Tensor, K: int, dtype) -> torch.Tensor:
    E = sum_bound(abs_terms, K)
    return E + rnd(ref.abs() + E, dtype)


def gelu_approx(z: torch.Tensor):
    """(approx of gelu, approx of gelu') of the module docstring, float64."""
    z = z.double()
    z2 = z * z
    e = torch.exp(-0.5 * z2)
    d_erf = 1.5e-7 + U32 + e * (57.0 + 3.0 * z2) * U32
    d_cdf = 0.5 * (d_erf + 2.0 * U32)
    cdf = 0.5 * (1.0 + torch.special.erf(z / np.sqrt(2.0)))
    pdf = e / np.sqrt(2.0 * np.pi)
    d_pdf = pdf * ((3.0 * z2 + 1.0) * U32 + 2.0 * U32)
    a_gelu = z.abs() * d_cdf + (z * cdf).abs() * U32
    a_grad = z.abs() * d_pdf + d_cdf + (cdf + z * pdf).abs() * U32
    return a_gelu, a_grad


def gelu_allowed(z: torch.Tensor, ref: torch.Tensor, which: int, dtype) -> torch.Tensor:
    a = gelu_approx(z)[which]
    return a + rnd(ref.abs() + a, dtype)


# ---- comparator -----------------------------------------------------------------------------------------------------------
def _coords(bad: torch.Tensor, limit=5):
    idx = torch.nonzero(bad)[:limit]
    if bad.dim() == 2:
        return [(int(m), int(n), int(m) // 128, int(n) // 256) for m, n in idx]
    return [tuple(int(v) for v in row) for row in idx]


def compare_exact(got: torch.Tensor, ref64: torch.Tensor, dtype, signed_zero=True):
    """Grid cases: got equals ref.to(dtype) BIT FOR BIT, the sign of a zero included (`reference` follows the kernels' IEEE
    operations in float64: an accumulator that starts at +0 gives +0 for an exactly cancelling sum, 0 times a negative factor
    is -0).  signed_zero=False compares values (+0 == -0): only for EPI_PATCH_PGD, whose clamps are fminf / fmaxf, and those may
    return either zero when both arguments are zeros.  Returns (violations, [(m, n, 128-row tile, 256-column tile), ...])."""
    if dtype in (torch.float16, torch.bfloat16):
        want, bits = round16(ref64, dtype), torch.int16
    else:
        want, bits = ref64.float(), torch.int32
        assert bool((want.double() == ref64).all()), "fp32 reference not exactly representable"
    assert got.dtype == want.dtype and got.shape == want.shape
    if signed_zero:
        bad = got.contiguous().view(bits) != want.contiguous().view(bits)
    else:
        bad = ~(got.double() == want.double())          # NaN in `got` is a violation
    return int(bad.sum()), _coords(bad)


def compare_bounded(got: torch.Tensor, ref64: torch.Tensor, allowed: torch.Tensor):
    """|got - ref| <= allowed per element.  Returns (violations, coordinates, largest error / allowed)."""
    err = (got.double() - ref64).abs()
    bad = ~(err <= allowed)
    ratio = float((err / allowed.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    return int(bad.sum()), _coords(bad), ratio
