"""The transforms of the training batch (``--warp``, ``--augment``, ``--mix``) as one chain: the fixed order, the three parsed flags,
one base seed, and one call per training step that takes the lengths, the step seed and the contiguous batch once and runs the
stages that are on (ops.warp, ops.augment, ops.mix: one launch each).  Training only: validation, test, saliency, the k-means
initialisation, the projection, the alignment fit and the artifact report never call it.  torch is imported in the call path only."""
from dataclasses import dataclass
from typing import Optional

import utils.augment
import utils.mix
import utils.warp
from utils.augment import AugmentSpec, step_seed
from utils.mix import MixSpec, mix_draws
from utils.warp import WarpSpec

ORDER = ("warp", "augment", "mix")                    # the order the stages run in: time warp, then augmentation, then the partner mix
_MODULES = {"warp": utils.warp, "augment": utils.augment, "mix": utils.mix}               # utils.<stage>.parse_<stage>


def parse_flags(args):
    """The three flags of an args namespace -> {stage: spec, or None when the stage is off}.  A namespace without a flag, and the
    text None / '' / none in any case, is off and never reaches the flag's parser; so is a flag whose values switch nothing on
    (twarp=0).  The regression task refuses --mix: its CRPS tails take one real-valued target per row."""
    specs = {}
    for name in ORDER:
        text = getattr(args, name, None)
        off = text is None or (isinstance(text, str) and text.strip().lower() in ('', 'none'))
        spec = None if off else getattr(_MODULES[name], "parse_" + name)(text)            # the parser is looked up per call
        specs[name] = spec if spec is not None and spec.active else None
    if specs["mix"] is not None and getattr(args, 'task_name', 'classification') == 'regression':
        raise ValueError("--mix with --task_name regression: mixup / CutMix mix class labels through the cross-entropy tails; "
                         "the CRPS tails have no soft-label form")
    return specs


@dataclass(frozen=True)
class TrainTransforms:
    """`warp` / `augment` / `mix`: the parsed flags, None when off; `base`: the base seed of utils.augment.step_seed for all three
    (None when all are off); `rank`: this process's, so that ranks draw differently.  False when no stage is on."""
    warp: Optional[WarpSpec] = None
    augment: Optional[AugmentSpec] = None
    mix: Optional[MixSpec] = None
    base: Optional[int] = None
    rank: int = 0

    @classmethod
    def from_args(cls, args, rank=0):
        """parse_flags(args), and the base seed: --seed when it is >= 0, else torch's initial seed (reading it does not advance the
        generator).  Rank 0 prints what is on.  Nothing is on: nothing beyond the flags' words is looked at."""
        specs = parse_flags(args)
        if not any(specs.values()):
            return cls(rank=rank)
        seed = int(getattr(args, 'seed', -1))
        if seed < 0:
            import torch
            seed = int(torch.initial_seed())
        for name, spec in specs.items():
            if spec is not None and rank == 0:
                print(f"{name}: {', '.join(f'{k}={v:g}' for k, v in spec._asdict().items() if v and (k != 'prob' or v != 1.0))}")
        return cls(base=seed, rank=rank, **specs)

    def __bool__(self):
        return self.base is not None

    def __call__(self, batch_x, label, padding_mask, train_step):
        """The training batch of step `train_step` on its device -> (batch, soft): the batch after the stages that are on, and the
        soft labels (label_b, lam) that _train_loss takes after `label` under --mix, else ().  Nothing on: the same tensor and
        nothing else -- no mask sum, no seed arithmetic, no launch, no draw.  Every stage works inside each sample's own length,
        the keep-mask's row sum, taken on the device without a host sync (an all-ones mask gives what no lengths give), and under
        the one seed step_seed(base, rank, step): ranks differ, the eager and the captured loop agree, no torch generator is
        consumed.  The padding, the mask, labels and regression targets stay as they are."""
        if not self:
            return batch_x, ()
        import torch
        from ign_hip import ops                       # the three ops are looked up per call
        lengths = padding_mask.sum(1).to(torch.int32)
        seed = step_seed(self.base, self.rank, train_step)
        batch_x, soft = batch_x.contiguous(), ()
        for name in ORDER:
            spec = getattr(self, name)
            if spec is None:
                continue
            if name == "warp":
                batch_x = ops.warp(batch_x, seed, lengths=lengths, **spec._asdict())
            elif name == "augment":
                batch_x = ops.augment(batch_x, seed, lengths=lengths, **spec._asdict())
            else:
                batch_x, soft = self._mix(ops, batch_x, label, lengths, seed)
        return batch_x, soft

    def _mix(self, ops, batch_x, label, lengths, seed):
        """The draws are made on the host (utils.mix.mix_draws) and reach the device from pinned memory without blocking.  Sample b
        is paired with (b + roll) mod B -- the loader has shuffled already; only CutMix, whose span depends on the length, reads the
        lengths back to the host (one small synchronising copy per step; mixup alone draws as for full lengths and never waits for
        the device)."""
        import torch
        B, T = batch_x.shape[0], batch_x.shape[1]
        cutmix = self.mix.cutmix > 0.0
        roll, lam, span = mix_draws(seed, B, lengths.cpu().numpy() if cutmix else T, self.mix)
        if batch_x.is_cuda:
            def put(a):
                return torch.from_numpy(a).pin_memory().to(batch_x.device, non_blocking=True)
        else:
            put = torch.from_numpy
        lam = put(lam)
        return ops.mix(batch_x, lam, roll, span=put(span) if cutmix else None, lengths=lengths), (label.roll(-roll), lam)
