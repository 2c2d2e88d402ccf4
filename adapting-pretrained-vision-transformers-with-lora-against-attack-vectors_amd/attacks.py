"""Attack facade with the reference's call signatures.

    batched_fgsm_attack(model, images, labels, epsilon, mean, std)   whitebox_attacks.py:22-38
    FGSM(model, eps) / PGD(model, eps, alpha, steps, random_start)   torchattacks, as used at
        .set_normalization_used(mean, std); attack(images, labels)   whitebox_attacks.py:110-113,169-170

All arithmetic runs in the HIP library: the forward/backward chain, the fused sign/project
step (vl_pgd_step), the random start (vl_pgd_init) and the whole PGD loop as one hipGraph per
iteration (vl_pgd_attack).

    APGD / APGDT / Square (torchattacks' signatures), AutoAttack (autoattack's, auto_attack.py:98-108) and run_suite: the built
    components of AutoAttack's standard L-inf suite -- APGD-CE (vl_apgd_attack), APGD-T (vl_apgdt_attack) and Square
    (vl_square_attack), each a device-resident loop.  FAB-T is not built.  The AutoAttack class itself still accepts only
    'apgd-ce' and 'square' (its refusals are pinned by tests); APGD-T is reached through APGDT and run_suite.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from .model import LogitsModel, ViTForImageClassification


def _unwrap(model) -> ViTForImageClassification:
    seen = 0
    while not isinstance(model, ViTForImageClassification):
        nxt = getattr(model, "model", None) or getattr(model, "base_model", None)
        if nxt is None or seen > 4:
            raise TypeError("attack needs a vitlora ViTForImageClassification (optionally inside LogitsModel / PeftModel)")
        model, seen = nxt, seen + 1
    return model


def _is_imagenet(mean, std) -> bool:
    from .engine import IMAGENET_MEAN, IMAGENET_STD
    m = [float(v) for v in torch.as_tensor(mean).flatten().tolist()]
    s = [float(v) for v in torch.as_tensor(std).flatten().tolist()]
    return all(abs(a - b) < 1e-6 for a, b in zip(m, IMAGENET_MEAN)) and all(abs(a - b) < 1e-6 for a, b in zip(s, IMAGENET_STD))


def batched_fgsm_attack(model, images, labels, epsilon, mean, std):
    """clamp(x + eps * sign(dCE/dx), 0, 1) with the model fed (x - mean) / std
    (whitebox_attacks.py:22-38).  One forward, CE, backward-to-input and one fused step: exactly one iteration of the PGD
    loop from x with alpha = eps and no random start (bit-identical: tests/test_hip_fullsize.py::test_fgsm_is_pgd1_...), so
    it runs as that -- one captured graph, and at the reference's batch of 32 two half-batch chains (vl_pgd_attack)."""
    vit = _unwrap(model)
    eng = vit._engine()
    vit.sync_params()
    m = [float(v) for v in torch.as_tensor(mean).flatten().tolist()]
    s = [float(v) for v in torch.as_tensor(std).flatten().tolist()]
    eng.set_normalization(m, s)
    x = images.detach().to(device=eng.device, dtype=torch.float32).contiguous()
    return eng.pgd_attack(x, labels, float(epsilon), float(epsilon), 1, random_start=False)


class _Attack:
    """The part of torchattacks.Attack the reference touches."""

    def __init__(self, model):
        self.model = model
        self._norm: Optional[tuple] = None      # set_normalization_used(mean, std)

    def set_normalization_used(self, mean: Sequence[float], std: Sequence[float]):
        """torchattacks contract: the inputs handed to the attack ARE normalised with (mean, std);
        they are mapped back to [0,1], attacked there with the model fed normalised pixels, and
        the result is normalised again.  (The reference calls this on UN-normalised images,
        whitebox_attacks.py:169-170 -- reproduced here by construction.)"""
        self._norm = ([float(v) for v in mean], [float(v) for v in std])

    def _prepare(self, images):
        vit = _unwrap(self.model)
        eng = vit._engine()
        vit.sync_params()                  # adapters written through torch since the last call: never attack stale operands
        x = images.detach().to(device=eng.device, dtype=torch.float32).contiguous()
        if self._norm is not None:
            mean, std = self._norm
            eng.set_normalization(mean, std)
            x = eng.channel_affine(x, std, mean)                 # inverse_normalize: x*std + mean
        return vit, eng, x

    def _finish(self, eng, adv):
        if self._norm is not None:
            mean, std = self._norm
            adv = eng.channel_affine(adv, [1.0 / s for s in std], [-m / s for m, s in zip(mean, std)], out=adv)
        return adv

    def __call__(self, images, labels):
        return self.forward(images, labels)


class FGSM(_Attack):
    """torchattacks.FGSM(model, eps): adv = clamp(x + eps * sign(grad), 0, 1)."""

    def __init__(self, model, eps=8 / 255):
        super().__init__(model)
        self.eps = eps

    def forward(self, images, labels):
        vit, eng, x = self._prepare(images)
        if self._norm is not None:            # the PGD loop feeds the model normalised pixels: one iteration of it, alpha = eps
            return self._finish(eng, eng.pgd_attack(x, labels, float(self.eps), float(self.eps), 1, random_start=False))
        eng.forward(x, normalise=False, train=False)
        eng.loss_ce(labels)
        gx, _ = eng.backward(True, False, tuple(x.shape))
        adv = x.clone()
        eng.pgd_step(adv, x, gx, self.eps, self.eps, 0.0, 1.0)
        return self._finish(eng, adv)


class PGD(_Attack):
    """torchattacks.PGD(model, eps, alpha, steps, random_start) (whitebox_attacks.py:112-113).
    `seed` seeds the library's counter-based random start (torch's RNG stream is not used)."""

    def __init__(self, model, eps=8 / 255, alpha=2 / 255, steps=10, random_start=True, seed=0):
        super().__init__(model)
        self.eps, self.alpha, self.steps, self.random_start, self.seed = eps, alpha, steps, random_start, seed
        self._calls = 0

    def forward(self, images, labels):
        vit, eng, x = self._prepare(images)
        if self._norm is None:
            # no normalisation registered: the model consumes the adversarial image as is
            eng.set_normalization([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
        adv = eng.pgd_attack(x, labels, self.eps, self.alpha, self.steps, self.random_start,
                             seed=self.seed + self._calls)
        self._calls += 1
        if self._norm is None:
            from .engine import IMAGENET_MEAN, IMAGENET_STD
            eng.set_normalization(IMAGENET_MEAN, IMAGENET_STD)   # back to the library default
        return self._finish(eng, adv)


def _apgd_ce(eng, x, labels, eps, steps, rho, n_restarts, seed, random_start=True):
    """APGD-CE with restarts on [0,1] images (the engine's normalisation is the caller's to set): starts from `x`, and an image
    that is classified correctly before the attack takes the misclassified point of the first restart that fools it.  Returns
    (adv, still_robust [B] bool, clean_correct [B] bool, result of the last restart)."""
    labels = labels.to(device=eng.device, dtype=torch.int64)
    correct = eng.forward(x, normalise=True).argmax(1) == labels
    robust = correct.clone()
    adv = x.clone()
    res = None
    for r in range(max(1, int(n_restarts))):
        res = eng.apgd_attack(x, labels, eps, steps, rho=rho, random_start=random_start, seed=int(seed) + r)
        take = robust & ~res["robust"]
        adv = torch.where(take.view(-1, 1, 1, 1), res["x_best_adv"], adv)
        robust = robust & res["robust"]
    return adv, robust, correct, res


class APGD(_Attack):
    """torchattacks.APGD(model, norm='Linf', eps, steps, n_restarts, seed, loss='ce', rho): Auto-PGD on cross-entropy, the
    whole loop on the device (vl_apgd_attack).  Restart r uses the library's counter-based random start with seed + r.
    The algorithm is the library's restatement of the autoattack package (include/vitlora.h): parity with the package is
    unpinned.  After a call `last` holds the last restart's x_best / x_best_adv / loss_best / robust."""

    def __init__(self, model, norm="Linf", eps=8 / 255, steps=10, n_restarts=1, seed=0, loss="ce", rho=0.75):
        super().__init__(model)
        if norm != "Linf":
            raise ValueError(f"APGD: only norm='Linf' is built (got {norm!r})")
        if loss != "ce":
            raise ValueError(f"APGD: only loss='ce' is built (got {loss!r})")
        self.norm, self.eps, self.steps, self.n_restarts, self.seed, self.loss, self.rho = norm, eps, steps, n_restarts, seed, loss, rho
        self.last = None

    def forward(self, images, labels):
        vit, eng, x = self._prepare(images)
        if self._norm is None:
            eng.set_normalization([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
        adv, _, _, self.last = _apgd_ce(eng, x, labels, self.eps, self.steps, self.rho, self.n_restarts, self.seed)
        if self._norm is None:
            from .engine import IMAGENET_MEAN, IMAGENET_STD
            eng.set_normalization(IMAGENET_MEAN, IMAGENET_STD)   # back to the library default
        return self._finish(eng, adv)


def _apgd_t(eng, x, labels, eps, steps, rho, n_target_classes, n_restarts, seed):
    """APGD-T on [0,1] images (the engine's normalisation is the caller's to set): every target class and restart and the fold
    over them run inside one library call (vl_apgdt_attack).  n_target_classes is capped by num_labels - 1.  Returns
    (adv, still_robust [B] bool, clean_correct [B] bool, the call's result dict)."""
    labels = labels.to(device=eng.device, dtype=torch.int64)
    k = max(1, min(int(n_target_classes), eng.arch.num_labels - 1))
    res = eng.apgdt_attack(x, labels, eps, steps, rho=rho, n_target_classes=k, n_restarts=max(1, int(n_restarts)), seed=int(seed))
    return res["x_adv"], res["robust"], res["clean_correct"], res


class APGDT(_Attack):
    """torchattacks.APGDT(model, norm='Linf', eps, steps, n_restarts, seed, eot_iter, rho, n_classes): targeted Auto-PGD on the DLR
    loss towards each of the n_target_classes = min(9, n_classes - 1) (capped by the model's num_labels - 1) most likely wrong
    classes, every run and the fold over runs on the device (vl_apgdt_attack).  An image counts as fooled when it is
    misclassified; hitting the target is not required.  Run k * n_restarts + r uses the library's counter-based random start with
    seed + that index.  The algorithm is the library's restatement of the autoattack package (include/vitlora.h, DESIGN.md section
    3.11): parity with the package is unpinned.  After a call `last` holds the result dict of Engine.apgdt_attack."""

    def __init__(self, model, norm="Linf", eps=8 / 255, steps=10, n_restarts=1, seed=0, eot_iter=1, rho=0.75, n_classes=10):
        super().__init__(model)
        if norm != "Linf":
            raise ValueError(f"APGDT: only norm='Linf' is built (got {norm!r})")
        if eot_iter != 1:
            raise ValueError(f"APGDT: only eot_iter=1 is built (got {eot_iter!r})")
        self.norm, self.eps, self.steps, self.n_restarts, self.seed, self.eot_iter, self.rho = norm, eps, steps, n_restarts, seed, eot_iter, rho
        self.n_classes = n_classes
        self.n_target_classes = min(9, int(n_classes) - 1)
        self.last = None

    def forward(self, images, labels):
        vit, eng, x = self._prepare(images)
        if self._norm is None:
            eng.set_normalization([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
        adv, _, _, self.last = _apgd_t(eng, x, labels, self.eps, self.steps, self.rho, self.n_target_classes, self.n_restarts, self.seed)
        if self._norm is None:
            from .engine import IMAGENET_MEAN, IMAGENET_STD
            eng.set_normalization(IMAGENET_MEAN, IMAGENET_STD)   # back to the library default
        return self._finish(eng, adv.clone())                    # (_finish normalises in place: `last` keeps the [0,1] point)


def _square(eng, x, labels, eps, n_queries, p_init, n_restarts, seed, image_offset=0, check_every=0):
    """Square with restarts on [0,1] images (the engine's normalisation is the caller's to set): an image that is classified
    correctly before the attack takes x_best of the first restart that fools it (restart r uses seed + r).  Returns
    (adv, still_robust [B] bool, clean_correct [B] bool, result of the last restart)."""
    labels = labels.to(device=eng.device, dtype=torch.int64)
    correct = eng.forward(x, normalise=True).argmax(1) == labels
    robust = correct.clone()
    adv = x.clone()
    res = None
    for r in range(max(1, int(n_restarts))):
        res = eng.square_attack(x, labels, eps, n_queries, p_init=p_init, seed=int(seed) + r, image_offset=image_offset,
                                check_every=check_every)
        take = robust & ~res["robust"]
        adv = torch.where(take.view(-1, 1, 1, 1), res["x_best"], adv)
        robust = robust & res["robust"]
    return adv, robust, correct, res


class Square(_Attack):
    """torchattacks.Square(model, norm='Linf', eps, n_queries, n_restarts, p_init, loss='margin', resc_schedule, seed): the
    score-based random-search attack of Andriushchenko et al. 2020, the whole loop on the device (vl_square_attack); it reads
    logits only, no gradient.  The algorithm is the library's restatement of the autoattack package's square.py from memory
    (include/vitlora.h): parity with the package is unpinned.  Two deliberate deviations: the window and
    its signs are drawn per image (the package: one window per batch), and the window is written as clamp(x0 +- eps, 0, 1)
    directly.  Restart r uses seed + r; an image takes the point of the first restart that fools it.  After a call `last`
    holds the last restart's x_best / margin_min / queries / robust."""

    def __init__(self, model, norm="Linf", eps=8 / 255, n_queries=5000, n_restarts=1, p_init=0.8, loss="margin",
                 resc_schedule=True, seed=0):
        super().__init__(model)
        if norm != "Linf":
            raise ValueError(f"Square: only norm='Linf' is built (got {norm!r})")
        if loss != "margin":
            raise ValueError(f"Square: only loss='margin' is built (got {loss!r})")
        if not resc_schedule:
            raise ValueError("Square: only the rescaled schedule (resc_schedule=True) is built")
        self.norm, self.eps, self.n_queries, self.n_restarts, self.p_init = norm, eps, n_queries, n_restarts, p_init
        self.loss, self.resc_schedule, self.seed = loss, resc_schedule, seed
        self.last = None

    def forward(self, images, labels):
        vit, eng, x = self._prepare(images)
        if self._norm is None:
            eng.set_normalization([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
        adv, _, _, self.last = _square(eng, x, labels, self.eps, self.n_queries, self.p_init, self.n_restarts, self.seed)
        if self._norm is None:
            from .engine import IMAGENET_MEAN, IMAGENET_STD
            eng.set_normalization(IMAGENET_MEAN, IMAGENET_STD)   # back to the library default
        return self._finish(eng, adv)


class AutoAttack:
    """autoattack.AutoAttack(model, norm='Linf', eps, version, attacks_to_run, seed) as auto_attack.py:98-108 uses it.
    Of the standard suite (APGD-CE, APGD-T, FAB-T, Square) this class runs the first and the last component: version='custom' runs
    any non-empty ordered subset of ['apgd-ce', 'square'], each component's result taken only for the images that are still robust;
    version='standard' raises NotImplementedError (FAB-T is not built; APGD-T is, and runs through run_suite below, which this
    class calls -- accepting 'apgd-t' here is a follow-up that goes with the tests that pin this class's refusals).  Images are in [0,1]; the model is fed
    (x - mean) / std (the reference wraps its model in a NormalizedModel, auto_attack.py:47-55), ImageNet constants unless
    `mean` / `std` are given.  Square draws per image from (seed, index of the image in x_orig): its result does not depend on bs."""

    BUILT = ("apgd-ce", "square")
    MISSING = ("apgd-t", "fab-t")

    def __init__(self, model, norm="Linf", eps=0.3, version="standard", attacks_to_run=(), seed=None, device=None, verbose=False,
                 steps=100, n_restarts=1, rho=0.75, mean=None, std=None, square_queries=5000, p_init=0.8, check_every=0):
        if norm != "Linf":
            raise ValueError(f"AutoAttack: only norm='Linf' is built (got {norm!r})")
        if version == "standard":
            raise NotImplementedError("AutoAttack(version='standard'): the standard suite runs APGD-T, FAB-T and Square after APGD-CE; "
                                      "APGD-T and FAB-T are not built; use version='custom', attacks_to_run=['apgd-ce', 'square']")
        if version != "custom":
            raise ValueError(f"AutoAttack: version must be 'standard' or 'custom' (got {version!r})")
        run = list(attacks_to_run)
        bad = [a for a in run if a not in self.BUILT]
        if bad or not run or len(set(run)) != len(run):
            raise NotImplementedError(f"AutoAttack: attacks_to_run must be a non-empty subset of {list(self.BUILT)} (not built: {bad})")
        self.model, self.norm, self.eps, self.version, self.attacks_to_run = model, norm, eps, version, run
        self.seed = 0 if seed is None else int(seed)
        self.steps, self.n_restarts, self.rho = steps, n_restarts, rho
        self.square_queries, self.p_init, self.check_every = square_queries, p_init, check_every
        from .engine import IMAGENET_MEAN, IMAGENET_STD
        self.mean = [float(v) for v in (mean if mean is not None else IMAGENET_MEAN)]
        self.std = [float(v) for v in (std if std is not None else IMAGENET_STD)]
        self.robust_accuracy = None

    def run_standard_evaluation(self, x_orig, y_orig, bs=250, image_offset=0):
        """image_offset: the index of x_orig[0] in the data set when a caller feeds the set in several calls (Square only)."""
        adv, self.robust_accuracy = run_suite(self.model, x_orig, y_orig, self.eps, attacks=self.attacks_to_run, bs=bs, seed=self.seed,
                                              steps=self.steps, n_restarts=self.n_restarts, rho=self.rho,
                                              square_queries=self.square_queries, p_init=self.p_init, check_every=self.check_every,
                                              mean=self.mean, std=self.std, image_offset=image_offset)
        return adv


def run_suite(model, x, y, eps, attacks=("apgd-ce", "apgd-t", "square"), bs=250, seed=0, steps=100, n_restarts=1, rho=0.75,
              n_target_classes=9, square_queries=5000, p_init=0.8, check_every=0, mean=None, std=None, image_offset=0):
    """The components of AutoAttack's standard L-inf suite that are built -- 'apgd-ce', 'apgd-t', 'square' -- in the order given,
    on images in [0,1] with the model fed (x - mean) / std (ImageNet constants unless given), in batches of `bs`.  Each component's
    result is taken only for the images the earlier components left robust.  'fab-t' raises NotImplementedError (not built).
    n_target_classes is capped by the model's num_labels - 1.  image_offset: the index of x[0] in the data set (Square draws per
    image index).  Returns (x_adv, robust_accuracy)."""
    run = list(attacks)
    for name in run:
        if name == "fab-t":
            raise NotImplementedError("run_suite: 'fab-t' is not built")
        if name not in ("apgd-ce", "apgd-t", "square"):
            raise ValueError(f"run_suite: unknown attack {name!r}")
    if not run or len(set(run)) != len(run):
        raise ValueError("run_suite: attacks must be a non-empty list without repeats")
    vit = _unwrap(model)
    eng = vit._engine()
    vit.sync_params()
    from .engine import IMAGENET_MEAN, IMAGENET_STD
    eng.set_normalization([float(v) for v in (mean if mean is not None else IMAGENET_MEAN)],
                          [float(v) for v in (std if std is not None else IMAGENET_STD)])
    x_all = x.detach().to(device=eng.device, dtype=torch.float32).contiguous()
    y_all = y.to(device=eng.device, dtype=torch.int64)
    out, n_robust = [], 0
    for lo in range(0, x_all.shape[0], int(bs)):
        xb, yb = x_all[lo:lo + bs], y_all[lo:lo + bs]
        adv = robust = None
        for name in run:
            if name == "apgd-ce":
                a, r, _, _ = _apgd_ce(eng, xb, yb, eps, steps, rho, n_restarts, seed)
            elif name == "apgd-t":
                a, r, _, _ = _apgd_t(eng, xb, yb, eps, steps, rho, n_target_classes, n_restarts, seed)
            else:
                a, r, _, _ = _square(eng, xb, yb, eps, square_queries, p_init, n_restarts, seed,
                                     image_offset=int(image_offset) + lo, check_every=check_every)
            if adv is None:
                adv, robust = a, r
            else:             # only for the images the earlier components left robust (r is False for clean-wrong images too)
                take = robust & ~r
                adv = torch.where(take.view(-1, 1, 1, 1), a, adv)
                robust = robust & r
        out.append(adv)
        n_robust += int(robust.sum().item())
    return torch.cat(out), n_robust / max(1, x_all.shape[0])


__all__ = ["batched_fgsm_attack", "FGSM", "PGD", "APGD", "APGDT", "Square", "AutoAttack", "run_suite", "LogitsModel"]
