"""CPU-only tests: the C-ABI library loads and exports every symbol of include/vitlora.h, the
host-side logic (peft target matching, key renaming, parameter counts, sharding) and the
data-parallel exchange step on the gloo backend with world_size 2."""
import importlib
import os
import re
import subprocess
import sys

import pytest
import torch

from helpers import O, PKG, ROOT, pkg


def header_functions():
    src = open(os.path.join(ROOT, "include", "vitlora.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vl_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_header_symbol():
    lib_mod = importlib.import_module(PKG + "._lib")
    names = header_functions()
    assert len(names) >= 25 and "vl_pgd_attack" in names and "vl_backward_lora" in names
    missing_sig = [n for n in names if n not in lib_mod.SIGNATURES]
    assert not missing_sig, f"ctypes binding lacks {missing_sig}"
    lib = lib_mod.load()            # raises if the .so is missing: there is no CPU fallback
    for n in names:
        assert hasattr(lib, n), n
    assert lib.vl_version().decode().startswith("vitlora-hip")
    assert set(lib_mod.SIGNATURES) - set(names) <= {"vl_bench_gemm"}   # binding has nothing the header lacks


ONCE_COMPILED_KERNELS = (
    "adam_kernel", "apgd_rand_init_kernel", "apgd_sched_kernel", "apgd_start_kernel", "apgd_step_kernel", "apgd_targets_kernel",
    "apgd_track_kernel", "apgdt_fold_kernel", "ce_loss_kernel", "ce_reduce_kernel", "channel_affine_kernel",
    "dlr_targeted_loss_kernel", "pgd_init_kernel", "pgd_step_kernel", "quantize_kernel", "square_init_kernel",
    "square_sched_kernel", "square_step_kernel", "square_track_kernel", "zero_kernel",
    "grad_scale_kernel", "classifier_grad_kernel", "dropout_mask_kernel", "merge_f32_kernel")


def test_precision_independent_kernels_are_compiled_once():
    """csrc/once_kernels.hip: the kernels that never touch a 16-bit operand exist ONCE in the library, not once per build of
    the 16-bit path (fp16 / bf16 operands: csrc/common.h).  Each kernel's host-side launch stub is one symbol of the .so."""
    import shutil
    if shutil.which("nm") is None:
        pytest.skip("nm not on PATH")
    out = subprocess.run(["nm", pkg().LIB_PATH], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    counts = {k: sum(1 for line in out.stdout.splitlines() if f"__device_stub__{k}E" in line) for k in ONCE_COMPILED_KERNELS}
    assert all(v == 1 for v in counts.values()), {k: v for k, v in counts.items() if v != 1}


def test_engine_refuses_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    P = pkg()
    with pytest.raises(P.VitLoraError):
        P.Engine(P.ArchConfig())


def test_target_resolution_and_key_renaming():
    P = pkg()
    assert P.resolve_targets(["query", "key", "value", "output.dense"]) == ("q", "k", "v", "o", "fc2")
    assert P.resolve_targets(["query", "value"]) == ("q", "v")
    assert P.resolve_targets(["intermediate.dense"]) == ("fc1",)
    assert P.resolve_targets([]) == ()
    assert P.canonical_key("vit.layers.3.attention.q_proj.weight") == "vit.encoder.layer.3.attention.attention.query.weight"
    assert P.canonical_key("vit.layers.0.attention.o_proj.bias") == "vit.encoder.layer.0.attention.output.dense.bias"
    assert P.canonical_key("vit.layers.11.mlp.fc2.weight") == "vit.encoder.layer.11.output.dense.weight"
    assert P.canonical_key("classifier.weight") == "classifier.weight"
    keys = P.expected_keys(P.ArchConfig())
    assert len(keys) == 8 + 12 * 16 and set(keys) == set(O.init_weights(O.OracleConfig()).keys())


def test_peft_parameter_count_known_answers():
    """infLora.ipynb:163, :919 -- r=4 / r=16 on query,value with the 101-class head saved."""
    pc = importlib.import_module(PKG + ".peft_compat")
    model_mod = importlib.import_module(PKG + ".model")
    P = pkg()

    class _Stub(pc.PeftModel):
        def __init__(self, arch, cfg):
            torch.nn.Module.__init__(self)
            self.config = cfg
            self._vit = type("V", (), {"arch": arch})()

    arch = P.ArchConfig(num_labels=101)
    c4 = pc.LoraConfig(r=4, lora_alpha=16, target_modules=["query", "value"], modules_to_save=["classifier"])
    assert _Stub(arch, c4).trainable_parameter_counts() == (225_125, 86_101_450)
    c16 = pc.LoraConfig(r=16, lora_alpha=16, target_modules=["query", "value"], modules_to_save=["classifier"])
    assert _Stub(arch, c16).trainable_parameter_counts() == (667_493, 86_543_818)
    c8 = pc.LoraConfig(task_type=pc.TaskType.SEQ_CLS, r=8, target_modules=["query", "key", "value", "output.dense"])
    tr, _ = _Stub(P.ArchConfig(num_labels=21), c8).trainable_parameter_counts()
    assert tr == 958_464 + 768 * 21 + 21
    assert model_mod.get_normalization("anything") == ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])


def test_shard_batch_partitions():
    opt = importlib.import_module(PKG + ".optim")
    for n, w in [(256, 8), (512, 8), (10, 3), (7, 8)]:
        spans = [opt.shard_batch(n, r, w) for r in range(w)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        sizes = [b - a for a, b in spans]
        assert max(sizes) - min(sizes) <= 1


def test_synthetic_weights_match_oracle_init():
    """bench.py's GPU weights (package synthetic.py) and its CPU baseline (oracle init) must be the same numbers."""
    syn = importlib.import_module(PKG + ".synthetic")
    P = pkg()
    arch = P.ArchConfig(image_size=64, hidden=128, layers=2, heads=2, mlp=256, num_labels=10)
    cfg = O.OracleConfig(image_size=64, hidden=128, layers=2, heads=2, mlp=256, num_labels=10)
    a, b = syn.random_state_dict(arch, seed=3), O.init_weights(cfg, seed=3)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    la, lb = syn.random_lora(arch, 8, ("q", "k", "v", "o", "fc2"), seed=4), O.init_lora(cfg, r=8, seed=4).ab
    assert la.keys() == lb.keys() and all(torch.equal(la[k][0], lb[k][0]) and torch.equal(la[k][1], lb[k][1]) for k in la)


def test_global_batch_plan_gives_every_rank_the_same_number_of_steps():
    """65 images, 2 ranks, batch 32: rank 0 used to run one more optimizer step than rank 1."""
    opt = importlib.import_module(PKG + ".optim")
    for n, batch, world in [(65, 32, 2), (64, 32, 2), (5, 4, 8), (100, 7, 3), (1, 32, 8)]:
        plans = [opt.global_batch_plan(n, batch, r, world, shuffle_seed=3) for r in range(world)]
        assert len({len(p) for p in plans}) == 1, (n, batch, world)
        steps = len(plans[0])
        assert steps == (n + batch - 1) // batch
        seen = []
        for st in range(steps):
            sizes = [len(p[st][0]) for p in plans]
            assert sum(sizes) == plans[0][st][1] and max(sizes) - min(sizes) <= 1
            assert len({p[st][1] for p in plans}) == 1
            for p in plans:
                seen += p[st][0]
        assert sorted(seen) == list(range(n))                 # every sample exactly once per epoch
    # same seed -> same order on every rank; another seed -> another order
    a = opt.global_batch_plan(50, 8, 0, 2, shuffle_seed=1)
    assert a == opt.global_batch_plan(50, 8, 0, 2, shuffle_seed=1) != opt.global_batch_plan(50, 8, 0, 2, shuffle_seed=2)


_WORKER_ODD = r'''
import os, sys, torch, importlib
import torch.distributed as dist
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
from helpers import O, PKG, make_case
opt = importlib.import_module(PKG + ".optim")
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:{port}", rank=int(sys.argv[1]), world_size=2,
                        timeout=__import__("datetime").timedelta(seconds=60))
rank = dist.get_rank()
N, BATCH = 9, 4                         # global batches of 4, 4, 1: the last one leaves rank 1 with an EMPTY shard
cfg, w, lora, x, y = make_case(batch=N, layers=1)
xn = O.normalise(x)
keys = None
steps = 0
for idx, n_global in opt.global_batch_plan(N, BATCH, rank, 2, shuffle_seed=11):
    if idx:
        _, _, g = O.lora_train_grads(w, cfg, xn[idx], y[idx], lora)            # mean over the LOCAL shard
        keys = sorted(g.keys(), key=str)
        flat = torch.cat([g[k].flatten() for k in keys])
    else:
        flat = torch.zeros(numel)                                               # empty shard: zero contribution
    numel = flat.numel()
    opt.allreduce_weighted_mean_(flat, len(idx), n_global)                      # the ONE exchange step
    # single-process gradient of the same global batch
    gidx = opt.global_batch_plan(N, BATCH, 0, 1, shuffle_seed=11)[steps][0]
    _, _, gf = O.lora_train_grads(w, cfg, xn[gidx], y[gidx], lora)
    ks = sorted(gf.keys(), key=str)
    full = torch.cat([gf[k].flatten() for k in ks])
    err = float((flat - full).norm() / full.norm())
    assert err < 1e-5, (steps, err)
    steps += 1
print("rank", rank, "steps", steps, flush=True)
assert steps == 3
dist.barrier(); dist.destroy_process_group()
'''


def test_data_parallel_ragged_last_batch_does_not_hang_gloo(tmp_path):
    """2 ranks, 9 samples, batch 4: every rank takes part in all 3 all-reduces (one of them with an empty shard) and
    the weighted exchange reproduces the single-process gradient of each global batch."""
    port = 31500 + (os.getpid() % 2000)
    script = tmp_path / "worker_odd.py"
    script.write_text(_WORKER_ODD.format(root=ROOT, port=port))
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert all("steps 3" in o for o in outs)


_WORKER = r'''
import os, sys, torch, importlib
import torch.distributed as dist
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
from helpers import O, PKG, make_case
opt = importlib.import_module(PKG + ".optim")
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:{port}", rank=int(sys.argv[1]), world_size=2)
rank = dist.get_rank()
cfg, w, lora, x, y = make_case(batch=6, layers=1)
xn = O.normalise(x)
lo, hi = opt.shard_batch(6, rank, 2)
_, _, g = O.lora_train_grads(w, cfg, xn[lo:hi], y[lo:hi], lora)          # mean over the LOCAL shard
keys = sorted(g.keys(), key=str)
flat = torch.cat([g[k].flatten() for k in keys])
opt.allreduce_mean_(flat)                                                  # the ONE exchange step
_, _, gf = O.lora_train_grads(w, cfg, xn, y, lora)                         # single-process full batch
full = torch.cat([gf[k].flatten() for k in keys])
err = float((flat - full).norm() / full.norm())
print("rank", rank, "rel err", err, flush=True)
assert err < 1e-5, err
dist.barrier(); dist.destroy_process_group()
'''


def test_data_parallel_gradient_exchange_gloo(tmp_path):
    """Sum of shard gradients (mean-reduced) == single-process gradient: the N > 1 train step's only
    collective, run on CPU tensors with gloo, world_size 2."""
    port = 29500 + (os.getpid() % 2000)
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, port=port))
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)


def test_pingpong_gemm_builds_without_vgpr_spills():
    """csrc/gemm_pp.hip keeps explicitly loaded operands in registers across steps (asm global_load + counted vmcnt): a
    spilled or copied destination register would be saved before its data arrives, so the build must not spill VGPRs."""
    import re
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    src = os.path.join(ROOT, PKG, "csrc", "gemm_pp.hip")
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-c", src,
                          "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", out.stderr)]
    assert len(spills) >= 5 and all(v == 0 for v in spills), spills
    # both builds (fp16 / bf16 operands) of it
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-DVL_BF16", "-c", src,
                          "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert all(int(x) == 0 for x in re.findall(r"VGPRs Spill: (\d+)", out.stderr))


def test_256_row_gemm_epilogues_on_the_path_build_without_vgpr_spills():
    """csrc/gemm256.hip sits at exactly 256 VGPRs.  A spilled register is reloaded behind an s_waitcnt vmcnt(0), which drains the
    LDS-DMA queue of the tile in flight (rounds 2-3: the GELU-forward instantiation carried three and lost ~6 %).  With the flags
    build.sh gives this file (the scheduler's AMDGPU register-pressure trackers; for the bf16 build relaxed-occupancy scheduling
    on top) every epilogue the ViT path launches on the 256-row kernel -- store, GELU, GELU-backward, residual add, patch
    forward -- must be spill-free in BOTH builds."""
    import re
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    src = os.path.join(ROOT, PKG, "csrc", "gemm256.hip")
    bs = open(os.path.join(ROOT, PKG, "csrc", "build.sh")).read()
    for tag, pat, extra in (("f16", r'gemm256:f16\|[^)]*\) echo "([^"]*)"', []), ("bf16", r'gemm256:bf16\) echo "([^"]*)"', ["-DVL_BF16"])):
        flags = re.search(pat, bs).group(1).split()
        out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"] + flags + extra +
                             ["-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        names = re.findall(r"Function Name: (\S+)", out.stderr)
        spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", out.stderr)]
        assert len(names) == len(spills) >= 16
        for n, v in zip(names, spills):
            m = re.search(r"gemm256_kernelILi(\d+)ELi(\d+)E", n)
            if m and int(m.group(2)) in (0, 2, 3, 4, 10):          # EPI_STORE_H16, GELU, GELU_BWD, PATCH_FWD, RESID_H16
                assert v == 0, (tag, n, v)


def test_perspective_warp_of_the_patch_overlay_host_and_oracle():
    """distortion_scale_max > 0 (patch_attack.py:95): the corner draw, the homography coefficients the host hands to
    vl_patch_apply_persp (patch.py) and the oracle's restatement of torchvision `perspective` (PARITY UNPINNED: torchvision is
    not installable) -- known answers that follow from the definition alone."""
    from oracle import patch_oracle as PO
    patch_mod = importlib.import_module(PKG + ".patch")
    S = 64
    corners = [[0, 0], [S - 1, 0], [S - 1, S - 1], [0, S - 1]]
    # identity: coefficients (1, 0, 0, 0, 1, 0, 0, 0); the warp returns the canvas
    q = patch_mod.perspective_coeffs(S, corners)
    assert max(abs(a - b) for a, b in zip(q, [1, 0, 0, 0, 1, 0, 0, 0])) < 1e-6
    img = torch.rand(1, 3, S, S, generator=torch.Generator().manual_seed(1))
    assert (PO.perspective(img, q) - img).abs().max().item() < 1e-4
    # the corner draw: deterministic per generator, inside the bands ART draws from
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    for dist_scale in (0.2, 0.5, 0.9):
        d = int(dist_scale * (S // 2))
        for _ in range(20):
            e = patch_mod.perspective_endpoints(S, dist_scale, g1)
            assert e == patch_mod.perspective_endpoints(S, dist_scale, g2)
            (tlx, tly), (trx, try_), (brx, bry), (blx, bly) = e
            assert all(0 <= v <= d for v in (tlx, tly, try_, blx)) and all(S - d - 1 <= v <= S - 1 for v in (trx, brx, bry, bly))
            # host coefficients == oracle coefficients (torch lstsq vs numpy lstsq), and each displaced corner reads its canvas corner
            qh, qo = patch_mod.perspective_coeffs(S, e), PO.perspective_coeffs(S, e)
            assert max(abs(a - b) for a, b in zip(qh, qo)) < 2e-5 * max(1.0, max(abs(v) for v in qo))
            for (xe, ye), (xs, ys) in zip(e, corners):
                den = qo[6] * xe + qo[7] * ye + 1
                assert abs((qo[0] * xe + qo[1] * ye + qo[2]) / den - xs) < 2e-3 and abs((qo[3] * xe + qo[4] * ye + qo[5]) / den - ys) < 2e-3
    # an axis-aligned shrink (corners move in by 8 pixels): the warp is a bilinear resize of the canvas into the inner square,
    # zero outside it; at the inner square's own corners it reads the canvas corners
    e = [[8, 8], [S - 9, 8], [S - 9, S - 9], [8, S - 9]]
    w = PO.perspective(img, PO.perspective_coeffs(S, e))
    assert w[..., :7, :].abs().max().item() == 0.0 and w[..., :, S - 7:].abs().max().item() == 0.0
    # torchvision evaluates the homography at pixel CENTRES (x + .5) and shifts back by .5 afterwards: inside the inner square
    # pixel x reads the canvas at (x + .5 - 8) * sc - .5, sc = (S - 1) / (S - 17) -- written here as a plain grid_sample
    sc = (S - 1) / (S - 17)
    pos = ((torch.arange(8, S - 8) + 0.5 - 8) * sc) / (0.5 * S) - 1.0
    grid = torch.stack(torch.meshgrid(pos, pos, indexing="xy"), dim=-1)[None]
    ref = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0]
    inner = w[0, :, 8:S - 8, 8:S - 8]
    assert (inner - ref).abs().max().item() < 2e-4


def test_integration_md_indexes_every_abi_symbol():
    """INTEGRATION.md section 3b lists EVERY entry point include/vitlora.h declares (with the reference callable it stands in for
    and its caller here), and nothing the header does not declare."""
    hdr = open(os.path.join(ROOT, "include", "vitlora.h")).read()
    syms = set(re.findall(r"\b(vl_[a-z0-9_]+)\s*\(", hdr))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("### 3b."):doc.index("## 4. Multi-GPU")]
    listed = set(re.findall(r"`(vl_[a-z0-9_]+)`", sec))
    assert syms - listed == set(), sorted(syms - listed)
    assert listed - syms == set(), sorted(listed - syms)


def test_integration_md_lists_every_environment_switch_and_csrc_reads_them_one_way():
    """INTEGRATION.md section 5 has one table row per VITLORA_* name that the library sources, the package's Python modules and the
    command-line scripts mention, and no row for a name none of them mentions; in csrc/ a switch is read through env.h
    (env_int / env_double / env_flag) -- the only other getenv calls are the three named helpers whose values are neither a
    flag nor an integer (VITLORA_RESID, VITLORA_ATTN_IMG: env_resid / env_attn_img of vitlora.hip; VITLORA_GRAPH_DUMP:
    env_graph_dump of vit_attacks.hip)."""
    import glob
    csrc = os.path.join(ROOT, PKG, "csrc")
    native = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    files = native + sorted(glob.glob(os.path.join(ROOT, PKG, "*.py")))
    files += [os.path.join(ROOT, n) for n in ("train.py", "train_loras.py", "whitebox_attacks.py", "eval_compose.py", "patch_attack.py")]
    used = set()
    for f in files:
        used |= set(re.findall(r"\bVITLORA_[A-Z0-9_]+", open(f).read()))
    assert len(used) > 30          # the scan found the sources
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 5. Environment switches"):]
    rows = re.findall(r"^\| `(VITLORA_[A-Z0-9_]+)` \|", sec, re.M)
    assert len(rows) == len(set(rows)), sorted(r for r in set(rows) if rows.count(r) > 1)
    assert used - set(rows) == set(), sorted(used - set(rows))
    assert set(rows) - used == set(), sorted(set(rows) - used)
    helpers = ("int env_resid() {", "int env_attn_img() {", "const char* env_graph_dump() {")
    stray = [(os.path.basename(f), line.strip()) for f in native if os.path.basename(f) != "env.h"
             for line in open(f) if "getenv(" in line and not line.strip().startswith(helpers)]
    assert stray == [], stray


def test_bench_dump_outputs_is_float32_bounded_and_repeatable(tmp_path, monkeypatch):
    """bench.py --dump-outputs (host side, no GPU): a small output is written whole; one above the limit as whole images of a
    seeded, sorted choice of batch indices that is the same on every call; always float32 and never above 64 MB."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    small = torch.rand(5, 3, 16, 16, generator=torch.Generator().manual_seed(0)).half()
    bench.dump_outputs(str(tmp_path / "s"), small)
    a = np.load(tmp_path / "s" / "adv.npy")
    assert a.dtype == np.float32 and np.array_equal(a, small.float().numpy())
    assert bench.DUMP_LIMIT_BYTES <= 64 << 20
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 16)  # the same rule at a size that costs nothing
    per = bench.DUMP_LIMIT_BYTES // 4 // 8                    # 8 images fit exactly, 19 do not
    big = torch.arange(19, dtype=torch.float32)[:, None].expand(19, per).contiguous()       # image i holds the value i
    bench.dump_outputs(str(tmp_path / "b1"), big)
    bench.dump_outputs(str(tmp_path / "b2"), big)
    b1, b2 = np.load(tmp_path / "b1" / "adv.npy"), np.load(tmp_path / "b2" / "adv.npy")
    assert b1.dtype == np.float32 and b1.shape == (8, per) and b1.nbytes <= bench.DUMP_LIMIT_BYTES
    assert np.array_equal(b1, b2)
    ids = b1[:, 0]
    assert (b1 == ids[:, None]).all() and (np.diff(ids) > 0).all() and set(ids) <= set(range(19))


def test_adam_drop_last_step_and_bench_flop_accounting():
    """Host logic added in round 5 (no GPU): (i) `optim.Adam.drop_last_step` takes a dropped optimizer step out of the
    bias-correction count, as an AMP skip-step never calls `optimizer.step()` (train_loras.py:314; round-4 ADVICE); (ii) the
    bench's algorithmic-FLOP functions: ViT-B/16 + LoRA r = 8 on q,k,v,o,fc2 = 72.438 GFLOP per image per PGD step
    and Swin-T + LoRA r = 16 = 19.43 (HF SwinConfig() shapes: 2 x 4.5 GMAC forward, dgrad once more, windowed attention x 2)."""
    import types
    optim = importlib.import_module(PKG + ".optim")
    p = torch.nn.Parameter(torch.zeros(8))
    opt = optim.Adam([p], lr=1e-3, model=None, distributed=False)
    opt.t = 5
    opt.drop_last_step()
    assert opt.t == 4
    opt.t = 0
    opt.drop_last_step()
    assert opt.t == 0                                       # never negative
    sys.path.insert(0, ROOT)
    import bench
    P = importlib.import_module(PKG)
    fl = bench.algorithmic_flops_per_image_step(P.ArchConfig(num_labels=21), 8, bench.TARGETS)
    assert abs(fl / 1e9 - 72.438) < 0.01, fl
    swin = importlib.import_module(PKG + ".swin")
    fs = bench.swin_flops_per_image_step(swin.SwinArch(num_labels=21), 16, bench.TARGETS)
    assert 19.0 < fs / 1e9 < 19.9, fs
    # forward alone without LoRA: 2 x the 4.35 GMAC the Swin paper quotes for Swin-T's linears + attention (4.5 GFLOPs "multiply-adds")
    f0 = bench.swin_flops_per_image_step(swin.SwinArch(num_labels=21), 0, ()) / 2
    assert 8.4e9 < f0 < 9.4e9, f0
