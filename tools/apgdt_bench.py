#!/usr/bin/env python3
"""ms per APGD-T attack against the APGD-CE attack of the same steps on the same GPU: ViT-B/16 + LoRA r = 8, f16, batch 256 and 32.

An APGD-T attack is one eval-mode forward (the clean pass that picks the targets), then n_target_classes * n_restarts APGD runs
of steps + 1 replays of {forward, dlr_targeted_loss_kernel, backward with the pixel gradient stored, apgd_track_kernel,
apgd_step_kernel}, each preceded by its random start and followed by apgdt_fold_kernel.  The expectation the tool checks is
time(APGD-T) = runs * time(APGD-CE with a random start) + one forward.

Method, as tools/apgd_bench.py: both forms are warmed up (graph capture and scratch included), then timed in turn, `--repeats`
rounds, each timing one attack between a device synchronise before and after (host clock); medians with the spread.
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
EPS = 8 / 255


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 32])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--n_target_classes", type=int, default=3)
    ap.add_argument("--n_restarts", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", default="f16")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("apgdt_bench needs the GPU: a CPU run cannot give a time")
    P = importlib.import_module(PKG)
    syn = importlib.import_module(PKG + ".synthetic")
    arch = P.ArchConfig(num_labels=21)
    eng = P.Engine(arch, P.LoraSpec(r=8, alpha=16.0, dropout=0.0, targets=TARGETS), precision=args.precision)
    eng.load_state_dict(syn.random_state_dict(arch, seed=0))
    for (i, t), (A, Bm) in syn.random_lora(arch, 8, TARGETS, seed=1).items():
        eng.param(i, t, "A").copy_(A)
        eng.param(i, t, "B").copy_(Bm)
    eng.plan(max(args.batches))                 # one plan: a later, larger one would drop the captured graphs
    n, runs = args.steps, args.n_target_classes * args.n_restarts
    out = {"arch": "vit_b16_lora_r8", "dtype": args.precision, "steps": n, "n_target_classes": args.n_target_classes,
           "n_restarts": args.n_restarts, "repeats": args.repeats, "batches": {}}
    for B in args.batches:
        x, y = syn.random_batch(arch, B, seed=100)
        x, y = x.cuda(), y.cuda()
        forms = {
            "apgd_t": lambda: eng.apgdt_attack(x, y, EPS, n, n_target_classes=args.n_target_classes, n_restarts=args.n_restarts, seed=1),
            "apgd_ce": lambda: eng.apgd_attack(x, y, EPS, n, random_start=True, seed=1),
            "forward": lambda: eng.forward(x, normalise=True),
        }
        times = {k: [] for k in forms}
        for f in forms.values():                # warm-up: code objects, the graph capture of this form, the scratch tensor
            f()
            f()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for k, f in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[k].append(1e3 * (time.perf_counter() - t0))
        res = {k: {"ms": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in times.items()}
        res["expected_apgd_t_ms"] = round(runs * res["apgd_ce"]["ms"] + res["forward"]["ms"], 3)
        res["apgd_t_ms_per_replay"] = round(res["apgd_t"]["ms"] / (runs * (n + 1)), 4)
        out["batches"][str(B)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
