"""Class weights and label smoothing of the training cross-entropy (``--class_weight``, ``--label_smoothing``): parsing, the
refusals ``run.get_args`` and ``Experiment`` share, the ``balanced`` weights and where the training labels of each provider live.

The weighted criterion is ``F.cross_entropy(z, y, weight=w, label_smoothing=eps)``: a mean over the batch divided by
``sum_b w[y_b]``, so a common scale of ``w`` cancels and the normalisation of ``balanced_weights`` only matters for reading them.
"""
import math

import numpy as np
import torch


def parse_class_weight(spec):
    """``--class_weight`` -> None (``none``), the string ``balanced``, or the list of floats of ``w0,w1,...``."""
    if spec is None or isinstance(spec, (list, tuple)):
        return None if spec is None else [float(v) for v in spec]
    text = str(spec).strip()
    if text.lower() in ('', 'none'):
        return None
    if text.lower() == 'balanced':
        return 'balanced'
    try:
        return [float(v) for v in text.split(',')]
    except ValueError:
        raise ValueError(f"--class_weight must be none, balanced or a comma list of numbers, got {spec!r}") from None


def check_weights(weights, num_class=None):
    """One positive finite value per class, or ValueError.  `num_class` None: the count is not known yet (checked again later)."""
    bad = [w for w in weights if not (math.isfinite(w) and w > 0)]
    if bad:
        raise ValueError(f"--class_weight: every weight must be positive and finite, got {bad[0]}")
    if num_class is not None and len(weights) != num_class:
        raise ValueError(f"--class_weight: {len(weights)} weights for {num_class} classes")


def check_loss_options(args, num_class=None):
    """The refusals of the two flags -> (parsed class weight, label smoothing).  Raises ValueError."""
    cw = parse_class_weight(getattr(args, 'class_weight', None))
    eps = float(getattr(args, 'label_smoothing', 0.0) or 0.0)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"--label_smoothing must be in [0, 1), got {eps}")
    if (cw is not None or eps != 0.0) and getattr(args, 'task_name', 'classification') == 'regression':
        raise ValueError("--class_weight / --label_smoothing with --task_name regression: the CRPS loss tail has no class weights")
    if isinstance(cw, list):
        check_weights(cw, num_class)
    return cw, eps


def balanced_weights(labels, num_class, notice=print):
    """-> float32 (num_class,) tensor: n / (N_present * count_c) for a class with samples (sklearn's "balanced", over the classes
    present), 1.0 for a class without any -- `notice` names those.  Labels outside [0, num_class) are not counted."""
    y = np.asarray(labels).reshape(-1).astype(np.int64)
    counts = np.bincount(y[(y >= 0) & (y < num_class)], minlength=num_class).astype(np.float64)
    present = counts > 0
    if not present.any():
        raise ValueError("balanced class weights need at least one training label")
    w = np.ones(num_class, dtype=np.float64)
    w[present] = counts.sum() / (present.sum() * counts[present])
    if not present.all() and notice is not None:
        notice(f"--class_weight balanced: no training sample of class(es) {np.flatnonzero(~present).tolist()}; their weight is 1.0")
    return torch.from_numpy(w.astype(np.float32))


def train_labels(dataset):
    """The labels of EVERY sample of a training dataset object (before any rank sharding): UEA (`labels_df`), the CHISCO .npy
    provider (`y` indexed by the split's `idx`) and SYNTH (`y`)."""
    if hasattr(dataset, 'labels_df'):
        return np.asarray(dataset.labels_df).reshape(-1)
    if hasattr(dataset, 'y') and hasattr(dataset, 'idx'):
        return np.asarray(dataset.y)[np.asarray(dataset.idx)]
    if hasattr(dataset, 'y'):
        return np.asarray(dataset.y).reshape(-1)
    raise ValueError(f"--class_weight balanced: {type(dataset).__name__} does not expose its training labels")


def resolve_class_weight(spec, dataset, num_class, notice=print):
    """The parsed flag -> None or the float32 (num_class,) host tensor of weights (checked: positive, finite, one per class)."""
    if spec is None:
        return None
    if spec == 'balanced':
        return balanced_weights(train_labels(dataset), num_class, notice)
    check_weights(spec, num_class)
    return torch.tensor(spec, dtype=torch.float32)
