"""CPU tests of tests/attn_ref.py itself: the comparator passes a float64 evaluation that rounds where the attention kernels
round (P and dS/scale to 16 bits, the outputs to 16 bits) and fails -- naming (image, head, token, column) -- on every fault
an attention kernel of this family could have, at every token count the GPU file runs, in fp16 and bf16; the derived bounds
hold with room for that evaluation; the ctypes mirror of vl_attn_case equals the header."""
import ctypes as C
import functools
import importlib
import math
import os
import re

import pytest
import torch

import attn_ref as A
from helpers import PKG, ROOT

T_FULL = [2, 17, 31, 32, 33, 63, 64, 65, 160, 192, 193, 197, 199, 200, 201, 223, 224]
T_CLS = T_FULL + [225, 256]
KINDS = ["permutation", "uniform", "continuous", "peaked_growing", "peaked_first"]
B, H, R, MODS = 2, 2, 4, 7


@functools.lru_cache(maxsize=None)
def prepared(kind, T, prec, cls):
    """case, reference, what a backward is given, and the criteria of both directions -- shared by every fault"""
    c = A.BUILDERS[kind](B, T, H, prec, seed=T, cls=cls, r=0 if cls else R, mods=MODS)
    ref = A.reference(c, prec)
    return c, ref, A.backward_inputs(c, ref, prec), A.expectations(c, ref, prec, "fwd"), A.expectations(c, ref, prec, "bwd")


def run(kind, T, prec, cls, direction, fault=None):
    c, ref, (ctx_in, lse_in), efwd, ebwd = prepared(kind, T, prec, cls)
    if direction == "fwd":
        return c, A.verify(c, A.emulate_forward(c, prec, fault), efwd, prec)
    return c, A.verify(c, A.emulate_backward(c, prec, ctx_in, lse_in, fault), ebwd, prec)


@pytest.mark.parametrize("prec", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("cls", [False, True], ids=["full", "cls"])
def test_comparator_passes_the_rounded_reference_and_the_bounds_hold_with_room(prec, cls):
    worst = 0.0
    for kind in KINDS:
        for T in (2, 32, 33, 197, 224) + ((256,) if cls else ()):
            for direction in ("fwd", "bwd"):
                _, (fails, ratios) = run(kind, T, prec, cls, direction)
                assert fails == [], (kind, T, direction, fails)
                worst = max([worst] + list(ratios.values()))
    assert worst < 1.0
    print(f"largest error / allowed of the rounded float64 evaluation ({prec}, {'cls' if cls else 'full'}): {worst:.3f}")


def applicable(fault, direction, cls):
    if fault in ("t_misses_a_head", "u_kv_exchanged"):
        return not cls
    if fault == "cls_dq_not_zeroed":
        return cls
    return True


CASES = [(d, f, cls) for d, fs in (("fwd", A.FAULTS_FWD), ("bwd", A.FAULTS_BWD)) for f in fs for cls in (False, True)
         if applicable(f, d, cls)]


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("direction,fault,cls", CASES, ids=[f"{d}-{f}-{'cls' if k else 'full'}" for d, f, k in CASES])
def test_every_fault_is_caught_at_every_token_count(direction, fault, cls, prec):
    """At least one operand kind must see the fault at EVERY token count, in both 16-bit types (a condition, not a measurement)."""
    for T in (T_CLS if cls else T_FULL):
        caught = None
        for kind in KINDS:
            c, (fails, _) = run(kind, T, prec, cls, direction, fault)
            if fails:
                caught = (kind, fails)
                break
        assert caught, f"{fault} ({direction}) at T = {T} in {prec}: no operand kind notices it"
        for name, n, where in caught[1]:                   # the report names (image, head, token, column)
            assert n > 0 and where and all(len(w) == 4 for w in where)
            for w in where:
                if name != "lse":
                    assert 0 <= w[0] < B and 0 <= w[2] < T and 0 <= w[3] < A.HD


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_the_report_names_the_damaged_place(prec):
    T = 65
    # one token row left unwritten: exactly that (image, token), every head and column
    c, (fails, _) = run("permutation", T, prec, False, "fwd", "row_unwritten")
    row = B * T // 2
    (name, n, where), = [f for f in fails if f[0] == "ctx"]
    assert n == H * A.HD and {(w[0], w[2]) for w in where} == {(row // T, row % T)}
    # two heads exchanged: every named element lies in head 0 or 1
    c, (fails, _) = run("continuous", T, prec, False, "bwd", "heads_exchanged")
    assert {f[0] for f in fails} == {"dq", "dk", "dv", "u"} and all(w[1] in (0, 1) for f in fails for w in f[2])
    # the stale lse entry: image 0, the last head, token T // 2 -- and nothing else
    c, (fails, _) = run("continuous", T, prec, False, "fwd", "lse_row_stale")
    assert fails == [("lse", 1, [(0, H - 1, T // 2, None)])]
    # key T counted: the permutation case sees it in the lse of the one query whose key is T - 1, per image and head
    c, (fails, _) = run("permutation", T, prec, False, "fwd", "key_T_valid")
    (name, n, where), = fails
    assert name == "lse" and n == B * H
    assert all(int(c.perm[w[1]][w[2]]) == T - 1 for w in where)


def test_structured_operands_have_the_properties_the_criteria_rest_on():
    for T in (2, 33, 200, 256):
        c = A.permutation_case(1, T, 2, "bf16", seed=T)
        ref = A.reference(c, "bf16")
        s = ref["Sraw"] * A.LOG2E / 8.0                                    # base-2 exponent units
        top = s.max(-1).values
        second = s.masked_fill(s == top.unsqueeze(-1), float("-inf")).max(-1).values
        assert bool((s.argmax(-1) == c.perm.unsqueeze(0)).all())
        assert T == 2 or float((top - second).min()) >= 40.0
        if T > 64:                                                         # pi moves tokens across 32-row tiles and 16-row halves
            moved = (c.perm // 32 != torch.arange(T) // 32).float().mean()
            assert float(moved) > 0.5 and bool(((c.perm // 16) % 2 != (torch.arange(T) // 16) % 2).any())
        u = A.uniform_case(1, T, 2, "bf16", seed=T)
        ru = A.reference(u, "bf16")
        assert bool((ru["P"] == 1.0 / T).all()) and float((ru["lse"] - math.log2(T)).abs().max()) < 1e-12


def test_ctypes_case_mirrors_the_header_struct():
    hdr = open(os.path.join(ROOT, "include", "vitlora.h")).read()
    body = re.search(r"typedef struct vl_attn_case \{(.*?)\} vl_attn_case;", hdr, flags=re.S).group(1)
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
    lib = importlib.import_module(PKG + "._lib")
    assert [(n, t) for n, t in lib.VLAttnCase._fields_] == fields
    names = dict(re.findall(r"#define VL_ATTN_(\w+) (\d+)", hdr))
    assert {k.upper(): str(v) for k, v in lib.ATTN_KERNELS.items()} == names
