"""AdamW, the per-step learning-rate schedule and the EMA of the weights (``--weight_decay``, ``--lr_schedule``, ``--ema``): the flags'
parsers and checks, and a numpy float64 restatement of the rule that ``csrc/ign_sched.h`` defines and ``ign_adamw_step_dev`` /
``ign_ema_update`` run on the flat buffers -- what the tests compare the kernels against.

    s = 1, 2, ...  the optimizer step (update s uses lr(s)); base = --lr, W warm-up steps, M the floor, S the run's optimizer steps
    s <  W              lr = base * s / W
    constant, s >= W    lr = base
    cosine,   s >= W    lr = M + (base - M) * 0.5 * (1 + cos(pi * t / T)),  t = min(s - W, T),  T = max(1, S - W)
    EMA                 d_s = min(D, (1 + s) / (10 + s));  ema += (1 - d_s) * (p - ema)
    AdamW               p *= 1 - lr(s) * WD  where the parameter decays, then the Adam update (torch.optim.AdamW)

No torch in this module.
"""
import math
from typing import NamedTuple

import numpy as np

KINDS = {'constant': 0, 'cosine': 1}            # IGN_SCHED_CONSTANT / IGN_SCHED_COSINE


class LrSchedule(NamedTuple):
    """The parsed ``--lr_schedule`` flag."""
    kind: str = 'none'
    warmup: int = 0
    min_lr: float = 0.0

    @property
    def active(self):
        return self.kind != 'none'

    @property
    def code(self):
        """The kernel's schedule kind; `none` is a constant schedule without warm-up."""
        return KINDS.get(self.kind, 0)


def parse_lr_schedule(spec):
    """``none`` / ``''`` / None, ``constant[,warmup=W]`` or ``cosine[,warmup=W][,min=M]`` -> LrSchedule.  W is an integer >= 0, M a
    finite number >= 0 (cosine only; that M <= --lr is check_optim_options' business).  Anything else raises ValueError."""
    if isinstance(spec, LrSchedule):
        return spec
    text = '' if spec is None else str(spec).strip()
    if text.lower() in ('', 'none'):
        return LrSchedule()
    kind, *items = [t.strip() for t in text.split(',')]
    if kind not in KINDS:
        raise ValueError(f"--lr_schedule: {kind!r} is not one of none|constant|cosine")
    keys = ('warmup', 'min') if kind == 'cosine' else ('warmup',)
    got = {}
    for item in items:
        key, eq, val = item.partition('=')
        key = key.strip()
        if not eq or key not in keys:
            raise ValueError(f"--lr_schedule {kind}: {item!r} is not one of {'|'.join(keys)}=VALUE")
        if key in got:
            raise ValueError(f"--lr_schedule: {key} given twice")
        try:
            got[key] = int(val) if key == 'warmup' else float(val)
        except ValueError:
            raise ValueError(f"--lr_schedule: {key}={val!r} is not {'an integer' if key == 'warmup' else 'a number'}") from None
    if got.get('warmup', 0) < 0:
        raise ValueError(f"--lr_schedule: warmup must be >= 0, got {got['warmup']}")
    m = got.get('min', 0.0)
    if not (math.isfinite(m) and m >= 0.0):
        raise ValueError(f"--lr_schedule: min must be finite and >= 0, got {m}")
    return LrSchedule(kind, got.get('warmup', 0), m)


def check_optim_options(args, flat_path=None):
    """-> (weight_decay, LrSchedule, ema) of an argparse namespace (one that predates the flags gives (0.0, none, 0.0)), refusing
    what cannot run: values out of range, two schedules at once, an average that a periodic projection would write behind, and --
    when the caller knows it (`flat_path` False) -- a device without the flat optimizer path."""
    wd = float(getattr(args, 'weight_decay', 0.0) or 0.0)
    ema = float(getattr(args, 'ema', 0.0) or 0.0)
    spec = parse_lr_schedule(getattr(args, 'lr_schedule', None))
    if not (math.isfinite(wd) and wd >= 0.0):
        raise ValueError(f"--weight_decay must be finite and >= 0, got {wd}")
    if not 0.0 <= ema < 1.0:
        raise ValueError(f"--ema must be in [0, 1), got {ema}")
    if spec.active and spec.min_lr > float(args.lr):
        raise ValueError(f"--lr_schedule: min={spec.min_lr} is above --lr {args.lr}")
    if spec.active and getattr(args, 'lr_decay', False):
        raise ValueError("--lr_schedule with --lr_decay: two learning-rate schedules at once; drop one")
    if ema > 0.0 and isinstance(getattr(args, 'shapelet_project', 'none'), int):
        raise ValueError("--ema with --shapelet_project N: the periodic projection writes the live shapelets mid-run and the "
                         "average would not follow; use --shapelet_project end")
    if (wd > 0.0 or spec.active or ema > 0.0) and flat_path is False:
        raise ValueError("--weight_decay / --lr_schedule / --ema run on the flat optimizer path of the GPU (FlatAdam); there is no "
                         "CPU optimizer twin")
    return wd, spec, ema


def total_steps(train_epochs, batches_per_epoch, accumulation=1):
    """S: the optimizer steps of a run -- a step closes whenever the run-wide batch count is a multiple of the accumulation."""
    return int(train_epochs) * int(batches_per_epoch) // max(int(accumulation), 1)


def lr_at(spec, base, total, s):
    """The learning rate of optimizer step s = 1, 2, ... in float64 (round to float32 once for the kernel's value)."""
    base = float(base)
    if s < spec.warmup:
        return base * s / spec.warmup
    if spec.kind != 'cosine':
        return base
    T = max(1, int(total) - spec.warmup)
    t = min(s - spec.warmup, T)
    return spec.min_lr + (base - spec.min_lr) * 0.5 * (1.0 + math.cos(math.pi * t / T))


def ema_decay_at(decay, s):
    """d_s = min(D, (1 + s) / (10 + s)): the usual warm-up of the decay, so that the average leaves the initial weights."""
    return min(float(decay), (1 + s) / (10 + s))


def adamw_reference(p, g, m, v, *, lr, step, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decay=None):
    """One torch.optim.AdamW step in float64 -> (p, m, v), new arrays.  `decay`: None (every element decays) or a boolean array
    like p (the per-element form of the kernel's chunk mask)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    if weight_decay != 0.0:
        keep = 1.0 - lr * weight_decay
        p = p * keep if decay is None else np.where(np.asarray(decay, dtype=bool), p * keep, p)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2_sqrt = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    return p - (lr / bc1) * m / (np.sqrt(v) / bc2_sqrt + eps), m, v


def ema_reference(ema, p, decay, s):
    """One EMA update in float64 -> the new average."""
    ema, p = np.asarray(ema, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return ema + (1.0 - ema_decay_at(decay, s)) * (p - ema)


def decays(name, param):
    """Whether --weight_decay shrinks this parameter.  Matrices and convolution kernels (ndim >= 2) do.  1-D tensors (biases,
    BatchNorm / LayerNorm affine parameters) do not.  Neither do the shapelet banks (``Shapelet.weights``) and the LTS thresholds
    (``threshold``): they are matched against instance-normalised windows, so shrinking them changes what a distance means (and
    fights --shapelet_project)."""
    if param.ndim < 2:
        return False
    return name.rsplit('.', 1)[-1] not in ('weights', 'threshold')


def decay_mask(names, params, offsets, n, align=64):
    """The kernel's mask: one uint8 per `align`-float chunk of a flat buffer of n floats whose parameter i starts at offsets[i] (a
    multiple of `align`); 1 where the chunk belongs to a parameter that decays, 0 elsewhere (the padding chunks included)."""
    mask = np.zeros((n + align - 1) // align, dtype=np.uint8)
    for name, p, off in zip(names, params, offsets):
        if off % align:
            raise ValueError(f"{name}: offset {off} is not a multiple of {align}")
        if decays(name, p):
            mask[off // align:(off + p.numel() + align - 1) // align] = 1
    return mask
