#!/usr/bin/env python3
"""AutoAttack's "auto" split on MI355X -- command-line compatible with the reference's auto_attack.py (flags: auto_attack.py:12-21;
directory layout <out>/<model>/<source>/<split>/auto/images/*.png + auto/metadata.csv: :60-68,112-115).

The reference runs AutoAttack(norm='Linf', eps, version='standard', seed=42) on every batch (:98-108).  Of that suite
(APGD-CE, APGD-T, FAB-T, Square) three components are built: APGD-CE (vl_apgd_attack: the whole Auto-PGD loop on the device),
APGD-T (vl_apgdt_attack: targeted Auto-PGD on the DLR loss, every target class and the fold over them on the device) and Square
(vl_square_attack: score-based random search on the logits, no gradient).  By default this script runs run_suite(attacks=
['apgd-ce']): an image that is classified correctly and that APGD-CE fools is replaced by the misclassified point, every other
image is written as it was.  --attacks apgd-ce apgd-t square runs each further component on the images the earlier ones leave
robust: APGD-T because cross-entropy saturates on an adapter that masks its gradients and the DLR ratio does not, Square as the
gradient-free cross-check.  FAB-T is not built.  All three are restatements of the package from memory: parity unpinned.
Extensions, all opt-in:
  --synthetic N           no dataset / checkpoint on disk: N seeded random images per split and seeded random-init weights.
  --arch tiny|vit_b|vit_l architecture of the checkpoint (default vit_b = google/vit-base-patch16-224).
  --precision f16|bf16|f32
  --steps K               APGD iterations (the package's standard version uses 100).
  --attacks A [A ...]     components to run in order, from apgd-ce, apgd-t and square (default: apgd-ce).
  --n_target_classes K    APGD-T's target classes per image (the package's standard version uses 9; at most num_classes - 1).
  --square_queries N      Square's query budget (the package's standard version uses 5000).
  --check_every K         Square looks at the robust flags every K queries and stops once every image is fooled (0 = never look).
"""
import argparse
import importlib
import os
import sys
import zlib

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
V = importlib.import_module("adapting-pretrained-vision-transformers-with-lora-against-attack-vectors_amd")


def build_parser():
    p = argparse.ArgumentParser(description="Generate AutoAttack (APGD-CE, APGD-T, Square; MI355X / HIP)")
    p.add_argument("--data_root", required=False, default=None)
    p.add_argument("--model", required=True, help="Model architecture name of the output tree (e.g., google_vit)")
    p.add_argument("--source", required=True, help="Source dataset (e.g., gtsrb)")
    p.add_argument("--model_path", required=False, default=None)
    p.add_argument("--output_dir", required=True)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--epsilon", type=float, default=0.031)
    p.add_argument("--splits", nargs="+", default=["train", "val", "test"])
    p.add_argument("--synthetic", type=int, default=0, metavar="N")
    p.add_argument("--num_classes", type=int, default=21, help="only with --synthetic")
    p.add_argument("--arch", choices=["tiny", "vit_b", "vit_l"], default="vit_b")
    p.add_argument("--precision", choices=["f16", "bf16", "f32"], default="f16")
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--attacks", nargs="+", choices=["apgd-ce", "apgd-t", "square"], default=["apgd-ce"])
    p.add_argument("--n_target_classes", type=int, default=9)
    p.add_argument("--square_queries", type=int, default=5000)
    p.add_argument("--check_every", type=int, default=0)
    return p


def load_model(args, device):
    syn = importlib.import_module(V.__name__ + ".synthetic")
    if args.synthetic:
        model = V.create_vit_model(args.num_classes, arch=syn.arch_by_name(args.arch, args.num_classes), device=device,
                                   precision=args.precision)
        model.load_state_dict(syn.random_state_dict(model.arch, seed=args.seed))
        return model.eval(), {f"class_{i}": i for i in range(args.num_classes)}
    iomod = importlib.import_module(V.__name__ + ".io")
    mapping_path = os.path.join(os.path.dirname(args.model_path), "class_mappings.txt")
    if not os.path.exists(mapping_path):
        raise FileNotFoundError(f"Class mapping file not found: {mapping_path}")
    class_to_idx = iomod.read_class_mappings(mapping_path)
    model = V.create_vit_model(len(class_to_idx), arch=syn.arch_by_name(args.arch, len(class_to_idx)), device=device,
                               precision=args.precision)
    model.load_state_dict(torch.load(args.model_path, map_location="cpu", weights_only=True))
    return model.eval(), class_to_idx


def batches(args, split, class_to_idx, model):
    """Yields (images in [0,1], labels, filenames)."""
    if args.synthetic:
        syn = importlib.import_module(V.__name__ + ".synthetic")
        x, y = syn.random_batch(model.arch, args.synthetic, seed=args.seed + zlib.crc32(split.encode()) % 1000)
        names = [f"{split}_{i:06d}.png" for i in range(args.synthetic)]
        for s in range(0, args.synthetic, args.batch_size):
            yield x[s:s + args.batch_size], y[s:s + args.batch_size], names[s:s + args.batch_size]
        return
    iomod = importlib.import_module(V.__name__ + ".io")
    meta = os.path.join(args.data_root, split, "metadata.csv")
    ds = iomod.FolderDataset(args.data_root, meta, class_to_idx, image_size=model.arch.image_size, sources=[args.source])
    loader = torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=False, num_workers=iomod.loader_workers(len(ds)),
                                         pin_memory=True)
    for images, labels, filenames in loader:
        yield images, labels, list(filenames)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.synthetic and not (args.data_root and args.model_path):
        raise SystemExit("--data_root and --model_path are required unless --synthetic N is given")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    print(f"Using device: {device}")
    iomod = importlib.import_module(V.__name__ + ".io")
    model, class_to_idx = load_model(args, device)
    mean, std = V.get_normalization(args.model)
    engine = model._engine()
    n_target = max(1, min(args.n_target_classes, len(class_to_idx) - 1))
    for split in args.splits:
        print(f"\nProcessing {split} split...")
        output_dir = os.path.join(args.output_dir, args.model, args.source, split, "auto", "images")
        os.makedirs(output_dir, exist_ok=True)
        seen, n_robust = [], 0
        for images, labels, filenames in batches(args, split, class_to_idx, model):
            images, labels = images.to(device), labels.to(device)
            offset = len(seen)                # Square draws by the image's index in the split, not by its place in the batch
            seen.extend(filenames)
            x_adv, robust_accuracy = V.run_suite(model, images, labels, args.epsilon, attacks=args.attacks, bs=args.batch_size,
                                                 seed=args.seed, steps=args.steps, n_target_classes=n_target,
                                                 square_queries=args.square_queries, check_every=args.check_every, mean=mean,
                                                 std=std, image_offset=offset)
            engine.check()                   # synchronises; fp16 mode: raises if a gradient left the fp16 range
            n_robust += round(robust_accuracy * len(filenames))
            iomod.save_images(x_adv, filenames, output_dir, engine=engine)
        if args.attacks == ["apgd-ce"]:
            print(f"  robust accuracy under APGD-CE (eps {args.epsilon:g}, {args.steps} steps): {n_robust}/{len(seen)}")
        else:
            budget = {"apgd-ce": f"{args.steps} steps", "apgd-t": f"{n_target} targets × {args.steps} steps",
                      "square": f"{args.square_queries} queries"}
            print(f"  robust accuracy under {' + '.join(args.attacks)} (eps {args.epsilon:g}, "
                  f"{', '.join(budget[a] for a in args.attacks)}): {n_robust}/{len(seen)}")
        if not args.synthetic:
            clean_meta = os.path.join(args.data_root, split, "metadata.csv")
            meta = iomod.create_adv_metadata(clean_meta, seen, output_dir)
            meta.to_csv(os.path.join(output_dir, "..", "metadata.csv"), index=False)
        print(f"AutoAttack ({' + '.join(a.upper() for a in args.attacks)}) results saved to: {os.path.dirname(output_dir)}")


if __name__ == "__main__":
    main()
