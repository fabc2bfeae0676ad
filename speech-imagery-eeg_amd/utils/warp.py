"""Time, magnitude and window warping of the training batch (``--warp``): the flag's parser and a numpy restatement of the rule that
``csrc/ign_warp.h`` defines and ``ign_warp_btc`` (``ops.warp``) runs -- what the tests compare the kernel against, bit for bit.

Sample b (n = its length) is resampled along time through a monotone map phi_b and scaled by a smooth gain curve g_b:

    out[b,t,c] = g_b(t) * lerp(x[b, i0, c], x[b, i0 + 1, c], w)     i0 = min(floor(phi_b(t)), n - 2), w = phi_b(t) - i0     t <  n
    out[b,t,c] = x[b,t,c]                                                                                              t >= n

phi_b is the window map (one window of the sample stretched or compressed by 2, the whole rescaled to [0, n - 1]) followed by the
smooth map (the integral of a piecewise-linear speed through K + 2 control values in 1 +- twarp, rescaled likewise); g_b is piecewise
linear through K + 2 control values in 1 +- mwarp, one curve for all channels.  Every draw is Philox4x32-10 under the 64-bit per-call
seed with the last counter word 3 (0..2 are utils/augment.py's), a pure function of (seed, b).  Every product, sum and quotient is
one float32 rounding, in the order the header writes them.  No torch in this module.
"""
from typing import NamedTuple

import numpy as np

from utils.augment import _key, philox4x32_10
from utils.flag_items import FlagItems

TAG_WARP = 3                                          # IGN_WARP_TAG
MAX_KNOTS = 8                                         # IGN_WARP_MAX_KNOTS
MAX_T = 1 << 20                                       # IGN_WARP_MAX_T: t * (K + 1) and the window integral stay exact in fp32
_F = np.float32
_SPEED, _GAIN = 1, 4                                  # first counter word 1 of the speed / gain knots


class WarpSpec(NamedTuple):
    """The parsed ``--warp`` flag; the field names are the keyword arguments of ``ops.warp``."""
    twarp: float = 0.0
    mwarp: float = 0.0
    wwarp: float = 0.0
    knots: int = 4
    prob: float = 1.0

    @property
    def active(self):
        return any(float(_F(v)) != 0.0 for v in (self.twarp, self.mwarp, self.wwarp))     # as the kernel sees the rates


_GRAMMAR = "none | twarp=R[,mwarp=R][,wwarp=R][,knots=K][,prob=P]"
_ITEMS = FlagItems("--warp", _GRAMMAR, ("twarp", "mwarp", "wwarp", "knots", "prob"))


def check_spec(twarp, mwarp, wwarp, knots, prob, who="--warp"):
    """The domain of the rule (what ign_warp_btc refuses with IGN_E_ARG): rates in [0, 1) as float32, knots 1..8, prob in (0, 1]."""
    for key, v in (("twarp", twarp), ("mwarp", mwarp), ("wwarp", wwarp)):
        if not 0.0 <= float(_F(v)) < 1.0:
            raise ValueError(f"{who}: {key} must be in [0, 1), got {v}")
    if int(knots) != knots or not 1 <= int(knots) <= MAX_KNOTS:
        raise ValueError(f"{who}: knots must be an integer in 1..{MAX_KNOTS}, got {knots}")
    if not 0.0 < float(_F(prob)) <= 1.0:
        raise ValueError(f"{who}: prob must be in (0, 1], got {prob}")


def parse_warp(spec):
    """``none`` / ``''`` / None, or ``twarp=0.2,mwarp=0.1,wwarp=0.1,knots=4,prob=0.5`` (any subset of the three rates, any order) ->
    WarpSpec.  The rates lie in [0, 1), knots in 1..8, prob in (0, 1]; knots / prob without a rate, unknown or repeated keys and
    values out of range raise ValueError."""
    if isinstance(spec, WarpSpec):
        return spec
    text = _ITEMS.clean(spec)
    if text is None:
        return WarpSpec()
    got = {}
    for key, val in _ITEMS.items(text):
        got[key] = _ITEMS.integer(key, val) if key == "knots" else _ITEMS.number(key, val)
    out = WarpSpec(**got)
    check_spec(*out)
    if not any(k in got for k in ("twarp", "mwarp", "wwarp")):
        raise ValueError(f"--warp: {text!r} names none of twarp / mwarp / wwarp{_ITEMS.tail}")
    return out


# --------------------------------------------------------------------------------------------------------- the rule, in numpy
def sample_draws(seed, b, n, wwarp, prob):
    """Per-sample draws of samples `b` with lengths `n` -> (on bool, a int64, Lw int64, c float32).  Lw = 0: no window map.
    A sample with n < 2 is never warped."""
    b, n = np.asarray(b, dtype=np.int64), np.asarray(n, dtype=np.int64)
    x0, x1, x2, _ = philox4x32_10(b, 0, 0, TAG_WARP, *_key(seed))
    u = (x0 >> np.uint64(8)).astype(_F) * _F(2.0 ** -24)
    on = (u < _F(prob)) & (n >= 2)
    win = (n >= 3) & (_F(wwarp) > 0)
    Lw = np.floor(_F(wwarp) * n.astype(_F)).astype(np.int64)
    Lw = np.where(win, np.minimum(np.maximum(Lw, 2), n - 1), 0)
    a = np.where(win, x1.astype(np.int64) % np.where(win, n - Lw + 1, 1), 0)
    c = np.where(win, np.where((x2 & np.uint64(1)) != 0, _F(2.0), _F(0.5)), _F(1.0)).astype(_F)
    return on, a, Lw, c


def knot_draws(seed, b, knots, first, rate):
    """Control values 0 .. knots + 1 of the speed (first = 1) or gain (first = 4) curve of sample b -> float32 (knots + 2,)."""
    i = np.arange(knots + 2)
    w = np.stack(philox4x32_10(b, first + (i >> 2), 0, TAG_WARP, *_key(seed)))           # (4, knots + 2)
    word = w[i & 3, i]
    u = (word >> np.uint64(8)).astype(_F) * _F(2.0 ** -24)
    return (_F(1.0) + _F(rate) * (_F(2.0) * u - _F(1.0))).astype(_F)


def _segment(p, n, knots):
    u = (p * _F(knots + 1)) / _F(n - 1)
    i = np.minimum(np.floor(u).astype(np.int64), knots)
    return i, u - i.astype(_F)


def warp_map(seed, b, n, spec=None, **kw):
    """The map of sample `b` with `n` steps of data -> (phi float32 (n,), gain float32 (n,)): ign_warp_map's, bit for bit.  An
    unwarped sample (prob, n < 2, every rate 0) has phi(t) = t and gain 1."""
    spec = WarpSpec(**kw) if spec is None else spec
    check_spec(*spec)
    twarp, mwarp, wwarp = (float(_F(v)) for v in spec[:3])                              # as the kernel sees the rates
    n, knots, prob = int(n), int(spec.knots), spec.prob
    t = np.arange(n, dtype=np.int64)
    phi, gain = t.astype(_F), np.ones(n, dtype=_F)
    if not spec.active or n < 2:
        return phi, gain
    on, a, Lw, c = (v[()] for v in sample_draws(seed, b, n, wwarp, prob))
    if not on:
        return phi, gain
    last = _F(n - 1)
    p = phi
    if Lw > 0:
        def integral(q):
            return q + (c - _F(1.0)) * np.minimum(np.maximum(q - _F(a), _F(0.0)), _F(Lw))
        p = (integral(p) * last) / integral(last)
    if twarp > 0.0:
        v = knot_draws(seed, b, knots, _SPEED, twarp)
        cum = np.zeros(knots + 2, dtype=_F)
        for j in range(knots + 1):                                                      # summed in order
            cum[j + 1] = cum[j] + _F(0.5) * (v[j] + v[j + 1])
        i, f = _segment(p, n, knots)
        integ = cum[i] + (f * v[i] + (f * f) * (_F(0.5) * (v[i + 1] - v[i])))
        p = (integ * last) / cum[knots + 1]
    phi = np.minimum(np.maximum(p, _F(0.0)), last).astype(_F)
    phi[n - 1] = last
    if mwarp > 0.0:
        m = knot_draws(seed, b, knots, _GAIN, mwarp)
        i, f = _segment(t.astype(_F), n, knots)
        gain = (m[i] + f * (m[i + 1] - m[i])).astype(_F)
    return phi, gain


def warp_reference(x, seed, lengths=None, *, twarp=0.0, mwarp=0.0, wwarp=0.0, knots=4, prob=1.0, first_sample=0):
    """The rule applied to a host float32 (B, T, C) array -> float32 array, bitwise what ops.warp gives.  `first_sample`: the batch
    index of row 0 (to restate a slice of a larger batch)."""
    x = np.asarray(x, dtype=_F)
    B, T, C = x.shape
    if T > MAX_T:
        raise ValueError(f"warp_reference: T={T} above {MAX_T}")
    spec = WarpSpec(twarp, mwarp, wwarp, knots, prob)
    check_spec(*spec)
    n_b = np.full(B, T, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, T)
    out = x.copy()
    if not spec.active:
        return out
    with np.errstate(invalid="ignore", over="ignore"):                                   # rows may hold inf / NaN on purpose
        for r in range(B):
            n = int(n_b[r])
            if n < 2 or not sample_draws(seed, r + first_sample, n, wwarp, prob)[0]:
                continue
            phi, gain = warp_map(seed, r + first_sample, n, spec)
            i0 = np.minimum(np.floor(phi).astype(np.int64), n - 2)
            w = (phi - i0.astype(_F))[:, None]
            x0, x1 = x[r, i0], x[r, i0 + 1]
            y = np.where(w == 0, x0, x0 + w * (x1 - x0))
            out[r, :n] = gain[:, None] * y if _F(mwarp) > 0 else y
    return out
