"""GPU tests of the one cache of captured attack iterations (csrc/vit_attacks.hip: GraphKey / GraphEntry, cached_graphs) that
vl_pgd_attack, vl_apgd_attack and vl_square_attack share, and of the scratch / workspace layouts behind it.

Everything runs on the tiny synthetic case (64 x 64 images, 2 layers, LoRA r = 8).  What is counted is "graph_captures": one per
cache ENTRY (a two-chain PGD entry holds two graphs and counts once).  Results are compared with torch.equal: a replayed graph
launches the kernels of the eager run with the same arguments, so nothing may differ."""
import os

import pytest
import torch

from helpers import make_case, make_engine

pytestmark = pytest.mark.gpu

EPS = 0.5 / 255
_S = {}


def case():
    if "case" not in _S:
        _S["case"] = make_case(image_size=64, r=8, batch=4, seed=5)
    return _S["case"]


def engine():
    """The shared f16 engine, planned for batch 4 once (a new plan would drop every cached graph)."""
    if "eng" not in _S:
        cfg, w, lora, _, _ = case()
        _S["eng"] = make_engine(cfg, w, lora)
        _S["eng"].plan(4)
    return _S["eng"]


def eager_engine():
    """A second engine created under VITLORA_NO_GRAPH=1: every attack on it runs eagerly, whatever the variable says later."""
    if "eager" not in _S:
        cfg, w, lora, _, _ = case()
        os.environ["VITLORA_NO_GRAPH"] = "1"
        try:
            _S["eager"] = make_engine(cfg, w, lora)
        finally:
            os.environ.pop("VITLORA_NO_GRAPH")
        _S["eager"].plan(4)
    return _S["eager"]


def cpu(r):
    torch.cuda.synchronize()
    if torch.is_tensor(r):
        return r.cpu()
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in r.items()}


def same(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    assert a.keys() == b.keys()
    return all(torch.equal(v, b[k]) if torch.is_tensor(v) else v == b[k] for k, v in a.items())


def own_scratch(nbytes):
    buf = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    return buf, (buf.data_ptr() + 255) // 256 * 256, nbytes


def test_the_cache_evicts_first_in_first_out_at_eight_entries():
    _, _, _, x, y = case()
    eng = engine()
    x, y = x[:2].cuda(), y[:2].cuda()
    eps = [(1 + i) / 255 for i in range(9)]
    pgd = lambda e: cpu(eng.pgd_attack(x, y, e, e, 1, random_start=False))        # noqa: E731  (alpha = eps: x0 +- eps)
    before = eng.counter("graph_captures")
    first = [pgd(e) for e in eps]
    assert eng.counter("graph_captures") == before + 9
    pgd(eps[8])
    assert eng.counter("graph_captures") == before + 9        # the newest entry is still there
    again = pgd(eps[0])
    assert eng.counter("graph_captures") == before + 10       # the oldest one was evicted by the ninth
    assert torch.equal(again, first[0])
    assert not torch.equal(first[0], first[8])                # (the nine attacks are different attacks)


def test_keys_of_the_three_attacks_do_not_collide():
    _, _, _, x, y = case()
    eng, ref = engine(), eager_engine()
    x, y = x.cuda(), y.cuda()

    def three(e):
        return [cpu(e.pgd_attack(x, y, EPS, EPS / 4, 2, random_start=False)), cpu(e.apgd_attack(x, y, EPS, steps=3, trace=True)),
                cpu(e.square_attack(x, y, EPS, n_queries=3, trace=True))]

    before = eng.counter("graph_captures")
    run1 = three(eng)
    assert eng.counter("graph_captures") == before + 3        # same batch and eps: one entry per kind all the same
    run2 = three(eng)
    assert eng.counter("graph_captures") == before + 3
    want = three(ref)
    assert ref.counter("graph_captures") == 0
    for name, a, b, w in zip(("pgd", "apgd", "square"), run1, run2, want):
        assert same(a, w), (name, "first run")
        assert same(b, w), (name, "second run")


def test_every_field_of_the_key_is_compared():
    _, _, _, x, y = case()
    eng = engine()
    x, y = x.cuda(), y.cuda()
    n = lambda: eng.counter("graph_captures")        # noqa: E731
    # APGD: rho alone differs (batch, eps, steps and the engine's cached scratch are the same)
    n0 = n()
    eng.apgd_attack(x, y, EPS, steps=4, rho=0.75)
    eng.apgd_attack(x, y, EPS, steps=4, rho=0.5)
    assert n() == n0 + 2
    eng.apgd_attack(x, y, EPS, steps=4, rho=0.75)
    assert n() == n0 + 2
    # PGD: alpha alone differs
    n0 = n()
    eng.pgd_attack(x, y, 3 * EPS, EPS, 1, random_start=False)
    eng.pgd_attack(x, y, 3 * EPS, EPS / 2, 1, random_start=False)
    assert n() == n0 + 2
    # Square: the scratch address alone differs
    nbytes = eng.square_scratch_bytes(4, 5)
    (buf_a, base_a, _), (buf_b, base_b, _) = own_scratch(nbytes), own_scratch(nbytes)
    assert base_a != base_b
    n0 = n()
    eng.square_attack(x, y, EPS, n_queries=5, scratch=(base_a, nbytes))
    assert n() == n0 + 1
    eng.square_attack(x, y, EPS, n_queries=5, scratch=(base_b, nbytes))
    assert n() == n0 + 2
    eng.square_attack(x, y, EPS, n_queries=5, scratch=(base_a, nbytes))
    assert n() == n0 + 2
    torch.cuda.synchronize()
    del buf_a, buf_b


# Layout facts of the tiny case, recorded from the library of commit 3a0777d (the parent of the commit that introduced the shared
# carver): (batch, n) -> (vl_apgd_scratch_bytes(batch, steps = n), vl_square_scratch_bytes(batch, n_queries = n),
# Engine.workspace_bytes(batch, train=False), Engine.workspace_bytes(batch, train=True)).  f16 and bf16 share every layout; the
# fp32 mode has its own activations and no half-batch chain workspaces.
SIZES = {
    "f16": {(1, 1): (297984, 150528, 3011328, 3789568), (3, 7): (887808, 445696, 9629440, 10407680),
            (32, 100): (9479936, 4786176, 26729728, 28974336)},
    "f32": {(1, 1): (297984, 150528, 2907648, 3595776), (3, 7): (887808, 445696, 3205120, 3893248),
            (32, 100): (9479936, 4786176, 17760768, 21201408)},
}
SIZES["bf16"] = SIZES["f16"]


@pytest.mark.parametrize("prec", ["f16", "bf16", "f32"])
def test_scratch_and_workspace_sizes_are_unchanged(prec):
    cfg, w, lora, _, _ = case()
    eng = make_engine(cfg, w, lora, precision=prec)
    for (batch, n), want in SIZES[prec].items():
        got = (eng.apgd_scratch_bytes(batch, n), eng.square_scratch_bytes(batch, n), eng.workspace_bytes(batch, False),
               eng.workspace_bytes(batch, True))
        assert got == want, (prec, batch, n)
