"""CPU tests of tests/gemm_ref.py itself: the comparator passes the correctly rounded reference and fails -- naming the damaged
tile -- on each subtle fault a GEMM kernel of this family could have; the Python dropout mask; the derived bounds; and the
ctypes mirror of vl_gemm_case against the header."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

import gemm_ref as G
from helpers import PKG, ROOT

M, N, K1, K2 = 256, 512, 128, 64


@pytest.fixture(scope="module")
def base():
    gen = torch.Generator().manual_seed(11)
    c = G.Case(epi="store_h16", A1=G.grid(gen, (M, K1)), W1=G.grid(gen, (N, K1)), A2=G.grid(gen, (M, K2)),
               W2=G.grid(gen, (N, K2)), bias=G.grid(gen, (N,)))
    return c, G.reference(c, torch.float16)


def ref_of(c, **changes):
    d = dict(c.__dict__)
    d.update(changes)
    return G.reference(G.Case(**d), torch.float16)["C"]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_comparator_passes_the_rounded_reference(base, dtype):
    c, ref = base
    assert G.compare_exact(G.round16(ref["C"], dtype), ref["C"], dtype) == (0, [])
    assert G.compare_exact(ref["C"].float(), ref["C"], torch.float32) == (0, [])
    G.exact_guard(ref["abs_z"], 2.0 ** -6)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_comparator_fails_on_each_subtle_fault_and_names_the_tile(base, dtype):
    c, ref = base
    good = G.round16(ref["C"], dtype)

    def verdict(bad):
        n, where = G.compare_exact(bad, ref["C"], dtype)
        assert n > 0
        return n, where

    # one element moved by one 16-bit ulp
    bad = good.clone()
    bad.view(torch.int16)[200, 300] += 1
    assert verdict(bad) == (1, [(200, 300, 1, 1)])
    # rows 127 and 128 swapped: the last row of tile row 0 and the first of tile row 1
    bad = good.clone()
    bad[[127, 128]] = good[[128, 127]]
    n, where = verdict(bad)
    assert {w[0] for w in where} <= {127, 128} and where[0][2] == 0 and n <= 2 * N
    # the last K tile of the main product left out
    n, where = verdict(G.round16(ref_of(c, A1=c.A1[:, :K1 - 64], W1=c.W1[:, :K1 - 64]), dtype))
    assert n > 0.9 * M * N and where[0][2:] == (0, 0)
    # the LoRA tile left out
    n, where = verdict(G.round16(ref_of(c, A2=None, W2=None), dtype))
    assert n > 0.9 * M * N
    # the bias of one 4-column group zeroed
    b = c.bias.clone()
    b[260:264] = 0
    n, where = verdict(G.round16(ref_of(c, bias=b), dtype))
    assert all(260 <= w[1] < 264 and w[3] == 1 for w in where) and n <= 4 * M
    # columns 16-31 of one tile exchanged with 32-47
    bad = good.clone()
    bad[128:256, 256 + 16:256 + 32], bad[128:256, 256 + 32:256 + 48] = good[128:256, 256 + 32:256 + 48], good[128:256, 256 + 16:256 + 32]
    n, where = verdict(bad)
    assert all(w[2] == 1 and w[3] == 1 and 256 + 16 <= w[1] < 256 + 48 for w in where)
    # the upper 32 columns of the LoRA tile dropped while they are nonzero
    w2 = c.W2.clone()
    w2[:, 32:] = 0
    n, where = verdict(G.round16(ref_of(c, W2=w2), dtype))
    assert n > 0.8 * M * N


def test_bounded_comparator_and_continuous_bound_arithmetic():
    """A CPU fp32 matmul of continuous operands stays far inside E (the issue measured under 2 %), passes the bound, and a
    result whose last K tile is missing does not."""
    gen = torch.Generator().manual_seed(12)
    for dtype in (torch.float16, torch.bfloat16):
        c = G.Case(epi="store_h16", A1=G.activations(gen, (M, K1), dtype), W1=G.weights(gen, (N, K1), dtype),
                   bias=0.1 * torch.randn(N, generator=gen))
        ref = G.reference(c, dtype)
        acc32 = c.A1.float() @ c.W1.float().T + c.bias
        E = G.sum_bound(ref["abs"], K1)
        assert float(((acc32.double() - ref["C"]).abs() / E).max()) < 0.05
        allowed = G.continuous_allowed(ref["C"], ref["abs"], K1, dtype)
        assert float((E / G.rnd(ref["C"].abs() + E, dtype)).median()) < 0.5      # at this depth the 16-bit rounding dominates
        n, _, ratio = G.compare_bounded(acc32.to(dtype), ref["C"], allowed)
        assert n == 0 and ratio <= 1.0
        short = (c.A1[:, :64].float() @ c.W1[:, :64].float().T + c.bias).to(dtype)
        n, where, ratio = G.compare_bounded(short, ref["C"], allowed)
        assert n > 0.9 * M * N and ratio > 10
        # a low mantissa bit of one operand lost: visible with these operands (it would not be on the grid)
        a = c.A1.clone()
        a.view(torch.int16)[:] &= ~1
        lossy = (a.float() @ c.W1.float().T + c.bias).to(dtype)
        assert G.compare_bounded(lossy, ref["C"], allowed)[0] > 0


def test_gelu_bound_holds_for_a_float64_evaluation_and_rejects_the_tanh_form():
    z = torch.linspace(-6, 6, 4801, dtype=torch.float64)
    cdf = 0.5 * (1 + torch.special.erf(z / 2 ** 0.5))
    ref = z * cdf
    a, ag = G.gelu_approx(z)
    assert float(a.max()) < 3e-5 and float(ag.max()) < 2e-5 and float(a.min()) >= 0      # a few fp32 ulps plus |z| * 0.75e-7
    allowed = G.gelu_allowed(z, ref, 0, torch.float16)
    assert G.compare_bounded(ref.to(torch.float16), ref, allowed)[0] == 0
    tanh = 0.5 * z * (1 + torch.tanh(0.7978845608 * (z + 0.044715 * z ** 3)))
    assert G.compare_bounded(tanh.to(torch.float16), ref, allowed)[0] > 0


def test_dropout_mask_values_and_keep_count():
    p, seed, stream = 0.1, 0x5EED, 3
    m = G.drop_mask(seed, stream, 128, 128, p)
    inv = G.inv_keep32(p)
    assert set(m.unique().tolist()) == {0.0, inv} and abs(inv - 1 / 0.9) < 1e-7
    kept = int((m != 0).sum())
    n = 128 * 128
    sigma = (n * p * (1 - p)) ** 0.5            # ~ 38
    assert abs(kept - n * (1 - p)) <= 6 * sigma
    # the vectorised form equals the integer restatement of common.h
    for idx in (0, 1, 127, 128, 5000, n - 1):
        assert bool(m.flatten()[idx] != 0) == G.drop_keep(seed, stream, idx, p)
    assert G.mix64(0) == 0xE220A8397B1DCDAF    # splitmix64's first output for seed 0 (published test vector)
    assert int((G.drop_mask(seed, stream, 128, 128, 0.5) != 0).sum()) not in (0, n)


def test_patch_index_maps_against_plain_loops():
    """The reshape that builds the image layout equals the per-element statement of gemm.h's patch epilogues."""
    gen = torch.Generator().manual_seed(13)
    ps, g, B = 4, 2, 3
    patches, T = g * g, g * g + 1
    c = G.Case(epi="patch_bwd", A1=G.grid(gen, (B * T, 64)), W1=G.grid(gen, (3 * ps * ps, 64)), M=128, Mvalid=B * patches,
               patches=patches, psize=ps, inv_std=(2.0, 4.0, 0.5), row_scale=torch.tensor([1.0, 0.5, 0.25]), a_gather=True)
    ref = G.reference(c, torch.float16)
    A, W = c.A1.double(), c.W1.double()
    for b in range(B):
        for p in range(patches):
            py, px = divmod(p, g)
            row = A[b * T + 1 + p]
            for n in range(3 * ps * ps):
                ch, rem = divmod(n, ps * ps)
                ph, pw = divmod(rem, ps)
                want = float(row @ W[n]) * c.inv_std[ch] * float(c.row_scale[b])
                assert float(ref["C"][b, ch, py * ps + ph, px * ps + pw]) == want


def test_ctypes_case_mirrors_the_header_struct():
    hdr = open(os.path.join(ROOT, "include", "vitlora.h")).read()
    body = re.search(r"typedef struct vl_gemm_case \{(.*?)\} vl_gemm_case;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    base = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(const )?(\w+)(\*?) (.*)", decl)
        ctype = C.c_void_p if m.group(3) else base[m.group(2)]
        for name in m.group(4).split(","):
            name = name.strip()
            arr = re.match(r"(\w+)\[(\d+)\]", name)
            fields.append((arr.group(1), ctype * int(arr.group(2))) if arr else (name, ctype))
    mirror = importlib.import_module(PKG + "._lib").VLGemmCase._fields_
    assert [(n, t) for n, t in mirror] == fields
