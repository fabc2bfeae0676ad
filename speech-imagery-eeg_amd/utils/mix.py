"""Mixup and CutMix along the time axis (``--mix``): the flag's parser, the per-step draws (made on the HOST), numpy restatements of
the batch rule that ``ign_mix_btc`` (``ops.mix``) runs and of the soft-label criterion that ``ign_loss_mix_fwd_bwd_reg``
(``ops.ign_loss(..., y_b=, lam=)``) runs, and the same criterion composed in torch for the models whose loss is torch's.

Batch rule, with partner p(b) = (b + roll) mod B, n_b = lengths[b] and span_b = (start_b, m_b):

    out[b,t,c] = x[p,t,c]                                      start_b <= t < start_b + m_b     (CutMix span, inside t < n_b)
    out[b,t,c] = lam_b * x[b,t,c] + (1 - lam_b) * x[p,t,c]     the other t < n_b                (a copy of x[b,t,c] at lam_b == 1)
    out[b,t,c] = x[b,t,c]                                      t >= n_b                         (padding copied through)

Criterion, with p = softmax(z), lp = log p, W = sum_n w_n, a_b = lam_b w[ya_b], c_b = (1 - lam_b) w[yb_b], D = sum_b (a_b + c_b):

    CEm = [ (1-eps) sum_b (a_b (-lp[b,ya_b]) + c_b (-lp[b,yb_b])) + (eps/N) sum_b sum_n w_n (-lp[b,n]) ] / D
    dCEm/dz[b,n] = [ (1-eps) (a_b (p_n - [n = ya_b]) + c_b (p_n - [n = yb_b])) + (eps/N) (p_n W - w_n) ] / D

lam == 1 everywhere is F.cross_entropy(weight=w, label_smoothing=eps); without weights it is
mean_b [lam_b CE(z_b, ya_b) + (1 - lam_b) CE(z_b, yb_b)].

Draws (mix_draws): one ``np.random.Generator(np.random.Philox(key=seed))`` per call, seed = utils.augment.step_seed(base, rank, step);
no torch generator is consumed.  Every array below has B entries and is drawn whether or not a sample uses it, so one sample's
decisions never move another's draws.  The order is fixed:

    1. word   = integers(0, 2^32)           roll = 1 + word mod (B - 1) for B >= 2, 0 for B == 1
    2. u_mix  = random(B)                    sample b is mixed when u_mix[b] < prob
    3. u_kind = random(B)                    with both mixup= and cutmix=: CutMix when u_kind[b] >= 0.5, else mixup
    4. beta(mixup, mixup, B)                 only when mixup= is given: lam of the mixup samples (float64, rounded to float32)
    5. beta(cutmix, cutmix, B)               only when cutmix= is given: lam' of the CutMix samples
    6. u_pos  = random(B)                    start = min(floor(u_pos (n - m + 1)), n - m), m = min(n, rint((1 - lam') n))
"""
from typing import NamedTuple

import numpy as np

from utils.flag_items import FlagItems


class MixSpec(NamedTuple):
    """The parsed ``--mix`` flag: the Beta parameters of mixup and CutMix (0 = off) and the chance that a sample is mixed."""
    mixup: float = 0.0
    cutmix: float = 0.0
    prob: float = 1.0

    @property
    def active(self):
        return self.mixup > 0.0 or self.cutmix > 0.0


_ITEMS = FlagItems("--mix", "mixup|cutmix|prob=VALUE", ('mixup', 'cutmix', 'prob'), need_value=False, expected=False,
                   strip_value=False)


def parse_mix(spec):
    """``none`` / ``''`` / None, or ``mixup=A[,cutmix=A][,prob=P]`` (any order; at least one of mixup= / cutmix=) -> MixSpec.
    A > 0 (finite) is the Beta(A, A) parameter, prob in (0, 1].  Unknown or repeated keys and values out of range raise ValueError."""
    if isinstance(spec, MixSpec):
        return spec
    text = _ITEMS.clean(spec)
    if text is None:
        return MixSpec()
    got = {}
    for key, val in _ITEMS.items(text):
        v = _ITEMS.number(key, val, finite=False)
        if key == 'prob':
            if not 0.0 < v <= 1.0:
                raise ValueError(f"--mix: prob must be in (0, 1], got {v}")
        elif not (np.isfinite(v) and v > 0.0):
            raise ValueError(f"--mix: {key} must be a finite Beta parameter > 0, got {v}")
        got[key] = v
    if 'mixup' not in got and 'cutmix' not in got:
        raise ValueError("--mix: prob= alone mixes nothing; give mixup=A and / or cutmix=A")
    return MixSpec(**got)


def mix_draws(seed, B, lengths, spec):
    """The draws of one training step -> (roll int, lam (B,) float32, span (B, 2) int32 = (start, m)); the order is the module
    docstring's.  `lengths`: the B sample lengths n_b (host integers), or one integer for all.  A mixup sample has an empty span
    (0, 0); a CutMix sample has lam = 1 - m / n_b, the share of it that is kept; an unmixed sample, and one with n_b = 0, has
    lam = 1 and an empty span."""
    spec = parse_mix(spec)
    B = int(B)
    n = np.broadcast_to(np.asarray(lengths, dtype=np.int64), (B,))
    if (n < 0).any():
        raise ValueError("mix_draws: negative length")
    rng = np.random.Generator(np.random.Philox(key=int(seed) & ((1 << 64) - 1)))
    word = int(rng.integers(0, 1 << 32, dtype=np.uint64))
    roll = 1 + word % (B - 1) if B >= 2 else 0
    mixed = rng.random(B) < spec.prob
    u_kind = rng.random(B)
    lam_mix = rng.beta(spec.mixup, spec.mixup, B) if spec.mixup > 0.0 else None
    lam_cut = rng.beta(spec.cutmix, spec.cutmix, B) if spec.cutmix > 0.0 else None
    u_pos = rng.random(B)
    cut = mixed & ((u_kind >= 0.5) if (lam_mix is not None and lam_cut is not None) else (lam_cut is not None))
    mup = mixed & ~cut
    lam = np.ones(B, dtype=np.float64)
    span = np.zeros((B, 2), dtype=np.int32)
    if lam_mix is not None:
        mup &= n > 0                                          # an empty sample has nothing to blend: lam = 1
        lam[mup] = lam_mix[mup]
    if lam_cut is not None:
        m = np.minimum(n, np.rint((1.0 - lam_cut) * n).astype(np.int64))
        start = np.minimum(np.floor(u_pos * (n - m + 1)).astype(np.int64), n - m)
        on = cut & (m > 0)                                    # m == 0 (also n == 0): nothing is cut, lam = 1
        lam[cut] = 1.0
        lam[on] = 1.0 - m[on] / n[on]
        span[on, 0], span[on, 1] = start[on], m[on]
    return roll, lam.astype(np.float32), span


def mix_reference(x, lengths, roll, lam, span):
    """The batch rule applied to a host (B, T, C) array in float32: bitwise what ign_mix_btc computes (1 - lam, the two products
    and the sum are separate fp32 roundings).  lengths / span may be None (full lengths / empty spans); both are clamped as the
    kernel clamps them."""
    x = np.asarray(x, dtype=np.float32)
    B, T, C = x.shape
    n = np.full(B, T, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, T)
    lam = np.asarray(lam, dtype=np.float32).reshape(B)
    if span is None:
        start, m = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    else:
        span = np.asarray(span, dtype=np.int64).reshape(B, 2)
        start = np.clip(span[:, 0], 0, n)
        m = np.clip(span[:, 1], 0, n - start)
    xp = x[(np.arange(B) + int(roll)) % B]
    t = np.arange(T, dtype=np.int64)[None, :]
    data = (t < n[:, None])[:, :, None]
    cut = ((t >= start[:, None]) & (t < (start + m)[:, None]))[:, :, None]
    l3 = lam[:, None, None]
    with np.errstate(invalid='ignore', over='ignore'):
        blend = l3 * x + (np.float32(1.0) - l3) * xp
    blend = np.where(l3 == np.float32(1.0), x, blend)
    return np.where(data, np.where(cut, xp, blend), x).astype(np.float32)


def mix_cross_entropy_reference(z, ya, yb, lam, weight=None, eps=0.0, grad=False):
    """The criterion CEm of the module docstring in float64 numpy -> the loss, or with `grad` (loss, dCEm/dz (B, N)) by the closed
    form (not autograd)."""
    z = np.asarray(z, dtype=np.float64)
    B, N = z.shape
    ya, yb = np.asarray(ya, dtype=np.int64).reshape(B), np.asarray(yb, dtype=np.int64).reshape(B)
    lam = np.asarray(lam, dtype=np.float64).reshape(B)
    w = np.ones(N) if weight is None else np.asarray(weight, dtype=np.float64).reshape(N)
    zs = z - z.max(1, keepdims=True)
    lp = zs - np.log(np.exp(zs).sum(1, keepdims=True))
    rows = np.arange(B)
    a, c = lam * w[ya], (1.0 - lam) * w[yb]
    D = (a + c).sum()
    loss = ((1.0 - eps) * (a * -lp[rows, ya] + c * -lp[rows, yb]).sum() + (eps / N) * (-lp * w[None, :]).sum()) / D
    if not grad:
        return loss
    p = np.exp(lp)
    hit_a, hit_b = np.zeros_like(p), np.zeros_like(p)
    hit_a[rows, ya], hit_b[rows, yb] = 1.0, 1.0
    g = ((1.0 - eps) * (a[:, None] * (p - hit_a) + c[:, None] * (p - hit_b)) + (eps / N) * (p * w.sum() - w[None, :])) / D
    return loss, g


def mix_cross_entropy(z, ya, yb, lam, weight=None, eps=0.0):
    """CEm composed in torch (differentiable; fp32 whatever the logits' dtype, as autocast does for a cross-entropy): the training
    criterion under --mix of the models whose loss is torch's (SBM, LTS, DNN, EEGCNN, and InterpGN under bf16 autocast)."""
    import torch
    lp = torch.log_softmax(z.float(), dim=-1)
    N = lp.shape[-1]
    lam = lam.to(lp.dtype)
    if weight is None:
        a, c = lam, 1.0 - lam
    else:
        weight = weight.to(lp.dtype)
        a, c = lam * weight[ya], (1.0 - lam) * weight[yb]
    nll = -(a * lp.gather(1, ya.unsqueeze(1)).squeeze(1) + c * lp.gather(1, yb.unsqueeze(1)).squeeze(1)).sum()
    if eps:
        smo = -(lp if weight is None else lp * weight).sum()
        nll = (1.0 - eps) * nll + (eps / N) * smo
    return nll / (a + c).sum()
