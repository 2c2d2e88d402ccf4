#!/usr/bin/env python3
"""ms per APGD iteration against ms per PGD iteration on the same GPU: ViT-B/16 + LoRA r = 8, f16, batch 256 and 32.

An APGD iteration is {forward, CE, backward with the pixel gradient stored to HBM, apgd_track_kernel, apgd_step_kernel} on one
chain; a PGD iteration of vl_pgd_attack fuses the step into the patch-gradient epilogue and, at batch 32, runs two half-batch
chains.  So three PGD forms are timed: the default, one chain with the fused step ("pgd_chains" = 1) and one chain with the
gradient stored and the separate pgd_step_kernel ("fuse_pgd" = 0) -- the last is APGD's chain without the bookkeeping.

Method: every form is warmed up (graph capture included), then the forms are timed in turn, `--repeats` rounds, each timing one
attack of `--steps` iterations between a device synchronise before and after (host clock); the median per form is reported, with
the spread.  An APGD attack of N steps replays N + 1 iterations (the start point is evaluated too): its time is divided by N + 1.
A timing tool, not a gate: prints one JSON line."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "adapting-pretrained-vision-transformers-with-lora-against-attack-vectors_amd"
TARGETS = ("q", "k", "v", "o", "fc2")
EPS, ALPHA = 8 / 255, 2 / 255


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 32])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", default="f16")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("apgd_bench needs the GPU: a CPU run cannot give a time")
    P = importlib.import_module(PKG)
    syn = importlib.import_module(PKG + ".synthetic")
    arch = P.ArchConfig(num_labels=21)

    def make(options):
        eng = P.Engine(arch, P.LoraSpec(r=8, alpha=16.0, dropout=0.0, targets=TARGETS), precision=args.precision)
        for k, v in options.items():            # before the first plan; a later change would drop the captured graphs
            eng.set_option(k, v)
        eng.load_state_dict(syn.random_state_dict(arch, seed=0))
        for (i, t), (A, Bm) in syn.random_lora(arch, 8, TARGETS, seed=1).items():
            eng.param(i, t, "A").copy_(A)
            eng.param(i, t, "B").copy_(Bm)
        return eng

    # one handle per form, so that no switch changes (and no graph is captured) inside a timed window
    e_default, e_fused, e_unfused = make({}), make({"pgd_chains": 1}), make({"pgd_chains": 1, "fuse_pgd": 0})
    n = args.steps
    out = {"arch": "vit_b16_lora_r8", "dtype": args.precision, "steps": n, "repeats": args.repeats, "batches": {}}
    for B in args.batches:
        x, y = syn.random_batch(arch, B, seed=100)
        x, y = x.cuda(), y.cuda()
        adv = torch.empty_like(x)

        def pgd(eng):
            return lambda: eng.pgd_attack(x, y, EPS, ALPHA, n, random_start=True, seed=1, out=adv)

        forms = {
            "apgd": (lambda: e_default.apgd_attack(x, y, EPS, n, random_start=True, seed=1), n + 1),
            "pgd_default": (pgd(e_default), n),
            "pgd_one_chain_fused": (pgd(e_fused), n),
            "pgd_one_chain_unfused": (pgd(e_unfused), n),
        }
        times = {k: [] for k in forms}
        for k, (f, _) in forms.items():          # warm-up: code objects, the graph capture of this form, the scratch tensor
            f()
            f()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for k, (f, iters) in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[k].append(1e3 * (time.perf_counter() - t0) / iters)
        out["batches"][str(B)] = {k: {"ms_per_iteration": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                                  for k, v in times.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
